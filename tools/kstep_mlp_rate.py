"""model_errors(..., mlp_kstep="batch") (one ampc_kstep_errors_mlp launch for any mix of shapes) against the default
mlp_kstep="shape" (one group per (hidden sizes, activation), one staged handle and one launch per model) for 64 MLP
configurations drawn by sample_mlp_config(np.random.default_rng(0)) at HalfCheetah dimensions (17 / 6), on a data set
of the size bench.py's `sub_records.model_axis` uses (40 trajectories x 201 rows of the c3 surrogate under random
controls; learning rates capped at 1e-3).  The models are fitted once with fit="device" (EPOCHS epochs) and scored at horizon 20 by both paths,
alternating in one process after one warm-up each; the host clock runs around calls that end in a synchronise.  A
"shape" repetition starts from models without a handle, as a tuner's fresh batch does: its handle staging
(ampc_set_mlp_dev: two packing kernels per model) is timed apart from its scoring.  The two score arrays must agree to
1e-9.
python tools/kstep_mlp_rate.py [repetitions] [--batch-only] [--small]
  --batch-only: the run rocprofv3 traces;  --small: score on the 4 held-out trajectories of a 10 % holdout instead."""
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: the device fit runs on torch's GPU)

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import zeros                                     # noqa: E402
from autompc_amd.evaluation import model_metrics as MM            # noqa: E402
from autompc_amd.synthetic import make_workload                   # noqa: E402
from autompc_amd.sysid.mlp import MLPFactory                      # noqa: E402
from autompc_amd.sysid.mlp_fit import fit_mlps                    # noqa: E402
from autompc_amd.tuning.configs import DictConfiguration, sample_mlp_config   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(ARGS[0]) if ARGS else 10
MODES = ("batch",) if "--batch-only" in sys.argv else ("shape", "batch")
N_MODELS, N_TRAJ, ROWS, EPOCHS, HORIZON = 64, 40, 201, 2, 20

system, task, surrogate, spec = make_workload("c3", precision="f64", device=0)
rng = np.random.default_rng(0)
nx, nu = system.obs_dim, system.ctrl_dim
X = rng.uniform(-0.1, 0.1, size=(N_TRAJ, nx))
trajs = [zeros(system, ROWS) for _ in range(N_TRAJ)]
for t in range(ROWS):                                             # the surrogate under random bounded controls
    U = rng.uniform(-1.0, 1.0, size=(N_TRAJ, nu))
    for k in range(N_TRAJ):
        trajs[k].obs[t], trajs[k].ctrls[t] = X[k], U[k]
    X = surrogate.pred_batch(X, U)
data = trajs[:4] if "--small" in sys.argv else trajs

cfg_rng = np.random.default_rng(0)
cfgs = [sample_mlp_config(cfg_rng) for _ in range(N_MODELS)]
for c in cfgs:
    c["lr"] = min(c["lr"], 1e-3)          # (the shapes are what is measured: no two-epoch fit at lr ~ 1 that diverges)
factory = MLPFactory(system, n_train_iters=EPOCHS, n_batch=64)
models = [factory(DictConfiguration(c), trajs, skip_train_model=True) for c in cfgs]
for m in models:
    m.jit_kernels = False
t0 = time.perf_counter()
info = fit_mlps(models, trajs, fit="device")
shapes = {MM.device_shape_key(m) for m in models}
print("%d MLPs fitted by the device fit in %.2f s (%d by its kernels): %d distinct shapes, depths %s, widths %d .. %d; "
      "scored on %d trajectories, %d start points, horizon %d"
      % (len(models), time.perf_counter() - t0, info["device_models"], len(shapes),
         sorted({len(m.hidden_sizes) for m in models}), min(min(m.hidden_sizes) for m in models),
         max(max(m.hidden_sizes) for m in models), len(data), int(MM.row_counts(data, 1)[0]), HORIZON), flush=True)


def run(mode):
    """(total seconds, staging seconds, scores, report)"""
    for m in models:
        m._invalidate()                                          # a fresh batch: no handle yet
    t0 = time.perf_counter()
    stage = 0.0
    if mode == "shape":
        for m in models:
            m._dev()                                             # ampc_create + ampc_set_mlp_dev
        models[-1]._dev().synchronize()
        stage = time.perf_counter() - t0
    out = MM.model_errors(models, data, [HORIZON], "rmse", mlp_kstep=mode)[:, 0]
    return time.perf_counter() - t0, stage, out, MM.last_report


for mode in MODES:                                                # warm-up: kernels loaded, allocator primed
    run(mode)
times, stages, out, reports = {m: [] for m in MODES}, [], {}, {}
for _ in range(REPS):
    for mode in MODES:
        t, st, out[mode], reports[mode] = run(mode)
        times[mode].append(t)
        if mode == "shape":
            stages.append(st)
assert reports["batch"].mlp_batch_calls == 1 and reports["batch"].mlp_batch_models == N_MODELS
assert all(m._handle is None for m in models) or "shape" in MODES
tb = statistics.median(times["batch"])
line = "batch: median %.4f s (min %.4f, max %.4f) over %d repetitions | %r" % (
    tb, min(times["batch"]), max(times["batch"]), REPS, reports["batch"])
if "shape" in MODES:
    ts, tst = statistics.median(times["shape"]), statistics.median(stages)
    diff = float(np.max(np.abs(out["batch"] / out["shape"] - 1)))
    line += ("\nshape: median %.4f s (min %.4f, max %.4f), of which handle staging %.4f s (min %.4f, max %.4f) | %r"
             "\nshape / batch = %.2f | max relative score difference %.2e"
             % (ts, min(times["shape"]), max(times["shape"]), tst, min(stages), max(stages), reports["shape"],
                ts / tb, diff))
    assert reports["shape"].device_models == N_MODELS and np.all(np.isfinite(out["shape"])) and diff <= 1e-9, \
        "the two paths disagree"
print(line, flush=True)
