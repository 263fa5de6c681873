"""IlqrCandidateEvaluator(mlp_models="table") (ONE iLQR plan with a model table for any mix of MLP shapes: the line
search, forward pass and Jacobian chain of csrc/ilqr_table_kernels.hpp) against the default mlp_models="shape" (one plan
per shape, side by side on host threads) for 64 iLQR candidates (random_ilqr_candidates) x 49 control steps at
HalfCheetah dimensions (17 / 6), max_iter 50.  The controller models are 64
configurations drawn by sample_mlp_config(np.random.default_rng(0)), fitted once with fit="device" (EPOCHS epochs,
learning rates capped at 1e-3) on 40 trajectories x 201 rows of the c3 surrogate under random controls; a batch uses the
first 64, 16 or 1 of them.  The two paths alternate in one process after one warm-up each; the host clock runs around
evaluate(), which ends in a synchronise.
python tools/ilqr_table_rate.py [repetitions] [--table-only]
  --table-only: the 64-shape table path alone (one warm-up, one timed evaluation), the run rocprofv3 --kernel-trace
                --stats traces.
  --kernel-stats <dir>: no GPU work; prints the per-kernel lines of the log from the *kernel_stats.csv that the
                rocprofv3 run below left under <dir>.
The whole measurement, each GPU step under its own time limit, log to profiles/ilqr_table_rate.log:
  timeout -k 10 420 python tools/ilqr_table_rate.py 5 && \
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/ilqr_table_rate.py --table-only && \
  python tools/ilqr_table_rate.py --kernel-stats <dir>
The log's last line (registers, scratch, LDS) is the compiler's: hipcc's -Rpass-analysis=kernel-resource-usage remarks for
launch_ilqr_table.cpp with the flags of csrc/build.py, and ilqr_table_lds_bytes (csrc/ilqr_table_host.hpp) at 17 / 6."""
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: the device fit runs on torch's GPU)

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import zeros                                          # noqa: E402
from autompc_amd.evaluation import model_metrics as MM                 # noqa: E402
from autompc_amd.synthetic import make_workload                        # noqa: E402
from autompc_amd.sysid.mlp import MLPFactory                           # noqa: E402
from autompc_amd.sysid.mlp_fit import fit_mlps                         # noqa: E402
from autompc_amd.tuning import IlqrCandidateEvaluator                  # noqa: E402
from autompc_amd.tuning.batch_eval import random_ilqr_candidates       # noqa: E402
from autompc_amd.tuning.configs import DictConfiguration, sample_mlp_config   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--") and a.isdigit()]
TABLE_ONLY = "--table-only" in sys.argv
REPS = 1 if TABLE_ONLY else (max(3, int(ARGS[0])) if ARGS else 5)
MODES = ("table",) if TABLE_ONLY else ("shape", "table")
N_MODELS, N_TRAJ, ROWS, EPOCHS = 64, 40, 201, 2

if "--kernel-stats" in sys.argv:
    import csv
    import glob
    where = sys.argv[sys.argv.index("--kernel-stats") + 1]
    files = sorted(glob.glob(where + "/**/*kernel_stats.csv", recursive=True))
    if not files:
        sys.exit("no *kernel_stats.csv under %s" % where)
    for r in list(csv.DictReader(open(files[0])))[:14]:
        print("%-62s calls %6s  total %12.1f (%5.1f %%)  avg %9.2f  min %9.2f  max %9.2f" % (
            r["Name"][:62], r["Calls"], float(r["TotalDurationNs"]) / 1e3, float(r["Percentage"]),
            float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    sys.exit(0)

system, task, surrogate, spec = make_workload("c3", precision="f64", device=0)
task.set_num_steps(50)
rng = np.random.default_rng(0)
nx, nu = system.obs_dim, system.ctrl_dim
X = rng.uniform(-0.1, 0.1, size=(N_TRAJ, nx))
trajs = [zeros(system, ROWS) for _ in range(N_TRAJ)]
for t in range(ROWS):                                                  # the surrogate under random bounded controls
    U = rng.uniform(-1.0, 1.0, size=(N_TRAJ, nu))
    for k in range(N_TRAJ):
        trajs[k].obs[t], trajs[k].ctrls[t] = X[k], U[k]
    X = surrogate.pred_batch(X, U)

cfg_rng = np.random.default_rng(0)
cfgs = [sample_mlp_config(cfg_rng) for _ in range(N_MODELS)]
for c in cfgs:
    c["lr"] = min(c["lr"], 1e-3)
factory = MLPFactory(system, n_train_iters=EPOCHS, n_batch=64)
models = [factory(DictConfiguration(c), trajs, skip_train_model=True) for c in cfgs]
for m in models:
    m.jit_kernels = False              # (what BatchPipelineTuner sets on the models it fits for one evaluation)
t0 = time.perf_counter()
info = fit_mlps(models, trajs, fit="device")
print("%d MLPs fitted by the device fit in %.2f s (%d by its kernels): %d distinct shapes, depths %s, widths %d .. %d"
      % (len(models), time.perf_counter() - t0, info["device_models"], len({MM.device_shape_key(m) for m in models}),
         sorted({len(m.hidden_sizes) for m in models}), min(min(m.hidden_sizes) for m in models),
         max(max(m.hidden_sizes) for m in models)), flush=True)

cands = random_ilqr_candidates(system, 64, seed=0)
evs = {mode: IlqrCandidateEvaluator(system, task, surrogate, mlp_models=mode) for mode in MODES}

for n_shapes in ((64,) if TABLE_ONLY else (64, 16, 1)):
    batch = [dict(c, model=models[i % n_shapes]) for i, c in enumerate(cands)]
    out, its, times = {}, {}, {m: [] for m in MODES}
    for mode in MODES:                                                 # warm-up: kernels loaded, allocator primed
        evs[mode].evaluate(batch)
    for _ in range(REPS):
        for mode in MODES:
            t0 = time.perf_counter()
            out[mode] = evs[mode].evaluate(batch)
            times[mode].append(time.perf_counter() - t0)
            its[mode] = int(np.sum(evs[mode].last_iterations)) if mode == "table" else -1   # (the shape groups keep no count)
            assert evs[mode].last_models["path"] == mode, evs[mode].last_models
    line = "%2d shapes, 64 candidates x 49 control steps, %d repetitions:" % (n_shapes, REPS)
    for mode in MODES:
        line += "\n  %-5s median %.4f s (min %.4f, max %.4f) | %r | finite scores %d%s" % (
            mode, statistics.median(times[mode]), min(times[mode]), max(times[mode]), evs[mode].last_models,
            int(np.isfinite(out[mode]).sum()), " | iLQR iterations %d" % its[mode] if its[mode] >= 0 else "")
    if not TABLE_ONLY:
        ok = np.isfinite(out["shape"]) & np.isfinite(out["table"])
        line += "\n  shape / table = %.2f | max relative score difference over the finite scores %.2e" % (
            statistics.median(times["shape"]) / statistics.median(times["table"]),
            float(np.max(np.abs(out["table"][ok] / out["shape"][ok] - 1))) if ok.any() else float("nan"))
    print(line, flush=True)
