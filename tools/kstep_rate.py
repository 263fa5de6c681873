#!/usr/bin/env python3
"""Rate of the k-step model-accuracy kernel (ampc_kstep_errors) on the MI355X.

Workload: HalfCheetah shape (17 obs, 6 ctrl), 25 holdout trajectories x 200 steps, horizons 1..20.
  one-shape   64 MLPs 2x256 relu in one call
  mixed       64 MLPs of shapes drawn by sample_mlp_config (one call per shape group)
Prints ms per model_errors call (wall, synchronised), model-steps/s and the algorithmic f64 FLOP rate
(2 * sum of layer in*out per model step) as a share of the 78.6 TF f64 MFMA peak.  Kernel-only time comes from
a separate `rocprofv3 --kernel-trace --stats -- python tools/kstep_rate.py --kernels-only` run.
Host comparison: the reference's loop (one pred_batch per trajectory, step and horizon) over the product's
pred_batch, timed on --host-models models and scaled to 64.  Tuner split: one BatchModelTuner batch of 64
configurations (HoldoutModelEvaluator, 100 trajectories, holdout 0.25), fit time vs metric time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_F64 = 78.6e12


def system_and_trajs(n_traj, T, seed):
    from autompc_amd import System, Trajectory
    system = System(["x%d" % i for i in range(17)], ["u%d" % i for i in range(6)], dt=0.05)
    rng = np.random.default_rng(seed)
    trajs = [Trajectory(system, T, 0.05 * rng.normal(size=(T, 17)).cumsum(axis=0), rng.normal(size=(T, 6)))
             for _ in range(n_traj)]
    return system, trajs


def make_models(system, cfgs):
    from autompc_amd import MLP
    out = []
    for k, c in enumerate(cfgs):
        kw = {key: v for key, v in c.items() if key != "lr"}
        m = MLP(system, seed=k, **kw)
        m.jit_kernels = False
        out.append(m)
    return out


def flops_per_step(m):
    dims = [m.system.obs_dim + m.system.ctrl_dim] + list(m.hidden_sizes) + [m.system.obs_dim]
    return 2.0 * sum(a * b for a, b in zip(dims[:-1], dims[1:]))


def time_call(fn, reps):
    fn()                                           # warm (handles staged, LDS attributes set)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-models", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true", help="the two device cases once each (for rocprofv3)")
    ap.add_argument("--train-iters", type=int, default=5)
    args = ap.parse_args()
    from autompc_amd.evaluation import model_errors
    from autompc_amd.evaluation.model_metrics import host_rmse, row_counts
    from autompc_amd.tuning.configs import sample_mlp_config
    system, trajs = system_and_trajs(25, 200, 0)
    hs = list(range(1, 21))
    rows = row_counts(trajs, 20)
    model_steps = float(rows.sum())                # counted (row, step) pairs per model; rows past rem run too
    run_steps = float(rows[0] * 20)                # what the kernel executes per model
    rng = np.random.default_rng(1)
    cases = {
        "one_shape": [{"n_hidden_layers": 2, "hidden_size": 256, "nonlintype": "relu"}] * 64,
        "mixed": [sample_mlp_config(rng) for _ in range(64)],
    }
    res = {"workload": {"obs": 17, "ctrl": 6, "trajectories": 25, "steps": 200, "horizons": "1..20",
                        "start_points": int(rows[0])}}
    for name, cfgs in cases.items():
        models = make_models(system, cfgs)
        f = sum(flops_per_step(m) for m in models)
        if args.kernels_only:
            model_errors(models, trajs, hs, "rmse")
            continue
        t = time_call(lambda: model_errors(models, trajs, hs, "rmse"), args.reps)
        res[name] = {"models": len(models), "shape_groups": len({(tuple(m.hidden_sizes), m.nonlintype) for m in models}),
                     "ms_per_call": 1e3 * t, "model_steps_per_s": len(models) * run_steps / t,
                     "tflop_per_call": f * run_steps / 1e12, "f64_tflops_wall": f * run_steps / t / 1e12,
                     "share_of_peak_wall": f * run_steps / t / PEAK_F64}
        if name == "one_shape":
            k = args.host_models
            t0 = time.perf_counter()
            for m in models[:k]:
                for h in hs:
                    host_rmse(m, trajs, h)
            th = (time.perf_counter() - t0) / k * len(models)
            res["host_composition"] = {"models_timed": k, "s_per_64_models_scaled": th, "device_speedup": th / t}
    if args.kernels_only:
        return
    # tuner split: one batch of 64 configurations
    from autompc_amd import MLPFactory
    from autompc_amd.evaluation import HoldoutModelEvaluator
    from autompc_amd.evaluation import evaluator as evmod
    from autompc_amd.sysid import mlp_fit
    from autompc_amd.tuning import BatchModelTuner
    _, data = system_and_trajs(100, 200, 2)
    split = {"fit_s": 0.0, "metric_s": 0.0}
    fit0, me0 = mlp_fit.fit_mlps, evmod.model_errors

    def fit_timed(*a, **k):
        t0 = time.perf_counter()
        try:
            return fit0(*a, **k)
        finally:
            split["fit_s"] += time.perf_counter() - t0

    def me_timed(*a, **k):
        t0 = time.perf_counter()
        try:
            return me0(*a, **k)
        finally:
            split["metric_s"] += time.perf_counter() - t0
    mlp_fit.fit_mlps, evmod.model_errors = fit_timed, me_timed
    try:
        ev = HoldoutModelEvaluator(system, data, "rmse", np.random.default_rng(3), horizon=20, holdout_prop=0.25)
        tuner = BatchModelTuner(system, ev, batch_size=64)
        tuner.add_model_factory(MLPFactory(system, n_train_iters=args.train_iters))
        t0 = time.perf_counter()
        cfgs = tuner.ask(64, np.random.default_rng(4))
        tuner.evaluate(cfgs)
        split["batch_s"] = time.perf_counter() - t0
    finally:
        mlp_fit.fit_mlps, evmod.model_errors = fit0, me0
    split.update(configurations=64, n_train_iters=args.train_iters, horizon=20, holdout_trajectories=len(ev.holdout))
    res["tuner_batch"] = split
    print(json.dumps(res))


if __name__ == "__main__":
    main()
