"""CandidateEvaluator(linear_models="table") (ONE MPPI plan with a table of ARX / Koopman models of any mix of state
dimensions: one rollout launch per control step, every model's update_state rule on the device,
csrc/mppi_linear_table_kernels.hpp) for 64 MPPI candidates x 49 control steps at CartPole shape (4 observations,
1 control) on an MLP surrogate.

  (a) Koopman   64 configurations drawn from KoopmanFactory's ranges (method lstsq) by default_rng(0), fitted once by
                fit_linear_models on 100 trajectories x 200 rows.  The table against the only way there was before it:
                one CandidateEvaluator per model (one lift per plan), each evaluating the candidates that carry its
                model -- in turn, and side by side on 8 host threads.
  (b) ARX, mix  64 ARX models of histories drawn from 1..10, and 32 of them with 32 of the Koopman models.  ONLY the
                table's time: before the table nothing could score an ARX controller model against a surrogate that is
                not itself on the device, so there is no other path to put next to it.

  (c) one wide  the 64 ARX models with the first replaced by a 252-state Koopman model: what one wide entry, which sets
                the launch's LDS reservation, costs the others.  The table's time only.

A batch uses the first 64, 16 or 1 of the models.  Next to every table time: the rollout and update kernels' mean time
per control step from HIP events, in one more evaluation.  The paths alternate in one process after one warm-up each; the host
clock runs around evaluate(), which ends in a synchronise.
python tools/linear_table_rate.py [repetitions] [--table-only]
  --table-only: the 64-model Koopman table path alone, the run rocprofv3 --kernel-trace --stats traces."""
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import ARX, MLP, Koopman, QuadCost, System, Task, Trajectory      # noqa: E402
from autompc_amd.sysid.linear_fit import fit_linear_models                        # noqa: E402
from autompc_amd.tuning import CandidateEvaluator, random_candidates              # noqa: E402
from autompc_amd.tuning.batch_eval import candidate_models                        # noqa: E402
from autompc_amd.tuning.configs import sample_arx_config, sample_koopman_config   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = max(5, int(ARGS[0])) if ARGS else 5
TABLE_ONLY = "--table-only" in sys.argv
N_MODELS, NO, NU = 64, 4, 1


def trajs(s, seed, n=100, L=200):
    """A damped nonlinear oscillator driven by random controls, scaled to |x| <= 0.8 (tools/sindy_table_rate.py)."""
    no, nu = s.obs_dim, s.ctrl_dim
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(no, no))
    M = np.eye(no) + 0.1 * (-0.4 * np.eye(no) + 0.5 * (S - S.T) / np.sqrt(no / 3.0))
    G = rng.normal(scale=0.3, size=(no, nu))
    raw = []
    for _ in range(n):
        obs, ctl = np.zeros((L, no)), rng.uniform(-0.5, 0.5, size=(L, nu))
        x = rng.uniform(-0.5, 0.5, size=no)
        for i in range(L):
            obs[i] = x
            x = M @ x + 0.4 * np.sin(2.0 * x[::-1]) + G @ ctl[i]
        raw.append((obs, ctl))
    scale = 0.8 / max(np.max(np.abs(o)) for o, _ in raw)
    return [Trajectory(s, L, scale * o, c) for o, c in raw]


system = System(["x%d" % i for i in range(NO)], ["u%d" % i for i in range(NU)], dt=0.05)
data = trajs(system, 1)
rng = np.random.default_rng(0)
koopmans = [Koopman(system, **sample_koopman_config(rng, methods=("lstsq",))) for _ in range(N_MODELS)]
arxs = [ARX(system, **sample_arx_config(rng)) for _ in range(N_MODELS)]
t0 = time.perf_counter()
rep = fit_linear_models(koopmans + arxs, data)
print("%d Koopman + %d ARX configurations fitted in %.2f s (host fits %d): Koopman states %d .. %d (%d distinct), ARX "
      "states %d .. %d (%d distinct)"
      % (len(koopmans), len(arxs), time.perf_counter() - t0, rep.host_fits, min(m.state_dim for m in koopmans),
         max(m.state_dim for m in koopmans), len({m.state_dim for m in koopmans}), min(m.state_dim for m in arxs),
         max(m.state_dim for m in arxs), len({m.state_dim for m in arxs})), flush=True)

task = Task(system)
task.set_cost(QuadCost(system, np.eye(NO), 0.01 * np.eye(NU), np.eye(NO)))
task.set_ctrl_bounds(np.full(NU, -0.5), np.full(NU, 0.5))
task.set_init_obs(np.array([0.2, -0.1, 0.1, 0.0]))
task.set_num_steps(50)
wrng = np.random.default_rng(3)
surrogate = MLP(system, n_hidden_layers=2, hidden_size_1=64, hidden_size_2=64, nonlintype="tanh")
surrogate.weights = [wrng.normal(scale=0.3, size=(64, NO + NU)), wrng.normal(scale=0.15, size=(64, 64)),
                     wrng.normal(scale=0.15, size=(NO, 64))]
surrogate.biases = [wrng.normal(scale=0.05, size=64), wrng.normal(scale=0.05, size=64), wrng.normal(scale=0.01, size=NO)]
surrogate.xu_means, surrogate.xu_std = np.zeros(NO + NU), np.ones(NO + NU)
surrogate.dy_means, surrogate.dy_std = np.zeros(NO), 0.05 * np.ones(NO)
cands = random_candidates(system, 64, seed=0)
for c in cands:
    c["Q"], c["R"], c["F"] = c["Q"] ** 0.25, c["R"] ** 0.25, c["F"] ** 0.25
table_ev = CandidateEvaluator(system, task, koopmans[0], surrogate=surrogate, linear_models="table")


def per_model(batch, threads):
    """The path before the table (Koopman only): one evaluator per model object, on the candidates that carry it."""
    ms, index = candidate_models(batch, koopmans[0])
    scores = np.empty(len(batch))

    def one(k):
        ids = np.nonzero(index == k)[0]
        # (models of more than 64 states roll out in 16-row tiles only; the others in the evaluator's default 32)
        ev = CandidateEvaluator(system, task, ms[k], surrogate=surrogate, tile_rows=16 if ms[k].state_dim > 64 else 32)
        scores[ids] = ev.evaluate([{key: v for key, v in batch[i].items() if key != "model"} for i in ids], seed=1,
                                  index_offset=ids)
    if threads > 1:
        with ThreadPoolExecutor(max_workers=threads) as pool:
            list(pool.map(one, range(len(ms))))
    else:
        for k in range(len(ms)):
            one(k)
    return scores


def measure(title, pool, paths, sizes):
    for n_models in sizes:
        batch = [dict(c, model=pool[i % n_models]) for i, c in enumerate(cands)]
        out, times = {}, {p: [] for p in paths}
        for p, run in paths.items():                                   # warm-up: kernels loaded, allocator primed
            run(batch)
        for _ in range(REPS):
            for p, run in paths.items():
                t0 = time.perf_counter()
                out[p] = run(batch)
                times[p].append(time.perf_counter() - t0)
        assert table_ev.last_models == {"path": "linear_table", "models": n_models, "plans": 1}, table_ev.last_models
        line = "%s, %2d models, 64 candidates x 49 control steps, %d repetitions:" % (title, n_models, REPS)
        for p in paths:
            line += "\n  %-9s median %.4f s (min %.4f, max %.4f) | finite scores %d" % (
                p, statistics.median(times[p]), min(times[p]), max(times[p]), int(np.isfinite(out[p]).sum()))
        if "in turn" in paths:
            ok = np.isfinite(out["table"]) & np.isfinite(out["in turn"])
            line += "\n  in turn / table = %.2f | 8 threads / table = %.2f | max relative score difference over the %d " \
                    "finite scores %.2e" % (statistics.median(times["in turn"]) / statistics.median(times["table"]),
                                            statistics.median(times["8 threads"]) / statistics.median(times["table"]),
                                            int(ok.sum()),
                                            float(np.max(np.abs(out["table"][ok] / out["in turn"][ok] - 1))) if ok.any()
                                            else float("nan"))
        tm = {}
        table_ev.evaluate(batch, seed=1, timing=tm)                    # (one more evaluation, its kernels bracketed by events)
        line += "\n  table, per control step (HIP events): rollout %.4f ms, update %.4f ms" % (
            tm["timing"]["rollout_ms"], tm["timing"]["update_ms"])
        print(line, flush=True)


TABLE = {"table": lambda b: table_ev.evaluate(b, seed=1)}
if TABLE_ONLY:
    measure("(a) Koopman", koopmans, TABLE, (64,))
else:
    measure("(a) Koopman", koopmans, dict(TABLE, **{"in turn": lambda b: per_model(b, 1),
                                                    "8 threads": lambda b: per_model(b, 8)}), (64, 16, 1))
    print("(b): the table's time only -- no other device path scores an ARX controller model against a surrogate that is "
          "not itself", flush=True)
    measure("(b) ARX", arxs, TABLE, (64, 16, 1))
    mix = [m for pair in zip(arxs[:32], koopmans[:32]) for m in pair]
    measure("(b) half ARX, half Koopman", mix, TABLE, (64,))
    # (c) what ONE wide entry costs the launch: the 64 ARX models with the first replaced by a 252-state Koopman model
    # (the launch reserves the [x | u] rows of its widest entry for every workgroup)
    wide = Koopman(system, trig_basis="true", trig_freq=31, strict_reference=False)
    wide.train(data, silent=True)
    measure("(c) ARX and one %d-state Koopman model" % wide.state_dim, [wide] + arxs[1:], TABLE, (64,))
