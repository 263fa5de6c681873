"""fit_mlps(..., fit="device") (the library's training kernels, ampc_mlpfit_*) against fit="torch" (the lockstep
PyTorch fit) on HalfCheetah-shaped data (17 states, 6 controls, 40 trajectories of 201 rows = 8000 training rows,
64-row mini-batches):

  (a) eight 2 x 256 relu models with their own seeds and learning rates -- the `model_axis` record's workload;
  (b) 64 MLP configurations drawn by sample_pipeline_configs(system, 64, rng, model_axis=True): depths 1-4, widths
      16-256, the four activations, their own learning rates.

Per path and workload one JSON line: groups, fit_s (wall time of the call, set-up and graph capture included), steps per
model, per-step microseconds (fit_s / steps: all models of the call advance one step) and where the models were fitted;
then the device path's speed-up.  Each path is warmed by a one-epoch fit of workload (a) first.

    python tools/mlp_fit_rate.py [--epochs 50] [--configs 64]
"""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import MLP, System, zeros                            # noqa: E402
from autompc_amd.sysid import mlp_fit                                 # noqa: E402
from autompc_amd.sysid.mlp import MLPFactory                          # noqa: E402
from autompc_amd.tuning import DictConfiguration, candidate_from_config, sample_pipeline_configs   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=50)
ap.add_argument("--configs", type=int, default=64)
args = ap.parse_args()

system = System(["x%d" % i for i in range(17)], ["u%d" % i for i in range(6)], dt=0.05)
rng = np.random.default_rng(0)
trajs = []
for _ in range(40):
    t = zeros(system, 201)
    t.obs[:] = 0.05 * rng.normal(size=(201, 17)).cumsum(axis=0)
    t.ctrls[:] = rng.uniform(-1, 1, size=(201, 6))
    trajs.append(t)


def eight(epochs):
    return [MLP(system, n_hidden_layers=2, hidden_size=256, nonlintype="relu", n_train_iters=epochs, n_batch=64,
                lr=1e-3 * (1 + 0.25 * k), seed=k) for k in range(8)]


def mixed(epochs):
    factory = MLPFactory(system, n_train_iters=epochs, n_batch=64)
    cfgs = sample_pipeline_configs(system, args.configs, np.random.default_rng(1), model_axis=True)
    return [factory(DictConfiguration(candidate_from_config(system, c)["model_cfg"]), trajs, skip_train_model=True)
            for c in cfgs]


results = {}
for how in ("torch", "device"):
    mlp_fit.fit_mlps(eight(1), trajs, fit=how)                        # warm-up: libraries, kernels' code objects
    for name, build in (("eight_2x256", eight), ("mixed_%d" % args.configs, mixed)):
        models = build(args.epochs)
        info = mlp_fit.fit_mlps(models, trajs, fit=how)
        rec = {"workload": name, "fit": how, "models": len(models), "epochs": args.epochs, "groups": info["groups"],
               "fit_s": round(info["fit_s"], 4), "steps": info["steps"],
               "us_per_step": round(1e6 * info["fit_s"] / info["steps"], 2),
               "device_models": info["device_models"], "torch_models": info["torch_models"]}
        results[(name, how)] = rec
        print(json.dumps(rec), flush=True)
for name in sorted({k[0] for k in results}):
    print(json.dumps({"workload": name,
                      "device_over_torch": round(results[(name, "torch")]["fit_s"] / results[(name, "device")]["fit_s"], 2)}))
