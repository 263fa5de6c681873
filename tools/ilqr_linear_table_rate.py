"""IlqrCandidateEvaluator(linear_models="table") (ONE iLQR plan with a table of ARX / Koopman models of any mix of state
dimensions: the sweep and the sixteen-row line search read a per-slot model, every model's update_state rule runs on
the device, csrc/ilqr_linear_table_kernels.hpp) for 64 iLQR candidates x 49 control steps at CartPole shape
(4 observations, 1 control) on an MLP surrogate.

  (a) Koopman   64 configurations drawn from KoopmanFactory's ranges (method lstsq) by default_rng(0), fitted once by
                fit_linear_models on 100 trajectories x 200 rows; batches of the first 64, 16 or 1 of them.  The table
                against the only way there was before it: per candidate, simulate() with the drop-in IterativeLQR (one
                device solve per control step, the host in between).  simulate() runs on the first --simulate candidates
                (default: all 64) and is scaled to 64.
  (b) ARX, mix  64 ARX models of histories drawn from 1..10, and 32 of them with 32 of the Koopman models: the table,
                and -- for the ARX batch -- one default evaluator per model in turn with every model ITS OWN surrogate
                (what the default path can score: another workload, the surrogate differs), next to the table.
  (c) kernels   the sweep and the line search per iteration (HIP events, ampc_ilqr_plan_set_timing) of a 64-problem
                queue on: the 64 ARX models; the same table with one 128-state entry that no problem uses (does one wide
                entry, which sets the launch's LDS reservation, cost the others?); a one-model table against the
                single-model plan on the same model (staged wide, and as ampc_set_linear stages it by itself).

The paths alternate in one process after one warm-up each; the host clock runs around evaluate(), which ends in a
synchronise.  Medians of the repetitions, with min and max.
python tools/ilqr_linear_table_rate.py [repetitions] [--simulate N]"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import ARX, MLP, IterativeLQR, Koopman, QuadCost, System, Task, Trajectory, _lib, simulate   # noqa: E402
from autompc_amd.sysid.linear_fit import fit_linear_models                        # noqa: E402
from autompc_amd.tuning import IlqrCandidateEvaluator, random_ilqr_candidates     # noqa: E402
from autompc_amd.tuning.batch_eval import candidate_models                        # noqa: E402
from autompc_amd.tuning.configs import sample_arx_config, sample_koopman_config   # noqa: E402

ARGS = sys.argv[1:]
N_SIM = int(ARGS[ARGS.index("--simulate") + 1]) if "--simulate" in ARGS else 64
POS = [a for i, a in enumerate(ARGS) if not a.startswith("--") and (i == 0 or ARGS[i - 1] != "--simulate")]
REPS = max(1, int(POS[0])) if POS else 5
N_MODELS, NO, NU, T = 64, 4, 1, 49


def trajs(s, seed, n=100, L=200):
    """A damped nonlinear oscillator driven by random controls, scaled to |x| <= 0.8 (tools/linear_table_rate.py)."""
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
task.set_num_steps(T + 1)
wrng = np.random.default_rng(3)
surrogate = MLP(system, n_hidden_layers=2, hidden_size_1=64, hidden_size_2=64, nonlintype="tanh")
surrogate.weights = [wrng.normal(scale=0.3, size=(64, NO + NU)), wrng.normal(scale=0.15, size=(64, 64)),
                     wrng.normal(scale=0.15, size=(NO, 64))]
surrogate.biases = [wrng.normal(scale=0.05, size=64), wrng.normal(scale=0.05, size=64), wrng.normal(scale=0.01, size=NO)]
surrogate.xu_means, surrogate.xu_std = np.zeros(NO + NU), np.ones(NO + NU)
surrogate.dy_means, surrogate.dy_std = np.zeros(NO), 0.05 * np.ones(NO)
cands = random_ilqr_candidates(system, 64, seed=0)
for c in cands:
    c["Q"], c["R"], c["F"] = c["Q"] ** 0.25, c["R"] ** 0.25, c["F"] ** 0.25
table_ev = IlqrCandidateEvaluator(system, task, koopmans[0], surrogate=surrogate, linear_models="table")


def by_simulate(batch):
    """The parent's only way to these scores: simulate() with the drop-in controller, candidate by candidate."""
    scores = np.full(len(batch), np.nan)
    for i, c in enumerate(batch[:N_SIM]):
        t1 = Task(system)
        t1.set_cost(QuadCost(system, np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"])))
        t1.set_ctrl_bounds(np.full(NU, -0.5), np.full(NU, 0.5))
        ctl = IterativeLQR(system, t1, c["model"], c["horizon"])
        ctl.reset()
        traj = simulate(ctl, task.get_init_obs(), task.term_cond, sim_model=surrogate, max_steps=T)
        scores[i] = task.get_cost()(traj)
    return scores


def own_surrogate_in_turn(batch):
    """One default evaluator per model, every model its own surrogate (ARX only): what the default path can score."""
    ms, index = candidate_models(batch, batch[0]["model"])
    scores = np.empty(len(batch))
    for k, m in enumerate(ms):
        ids = np.nonzero(index == k)[0]
        ev = IlqrCandidateEvaluator(system, task, m)
        scores[ids] = ev.evaluate([{key: v for key, v in batch[i].items() if key != "model"} for i in ids])
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
        line = "%s, %2d models, 64 candidates x %d control steps, %d repetitions:" % (title, n_models, T, REPS)
        for p in paths:
            line += "\n  %-22s median %.4f s (min %.4f, max %.4f) | finite scores %d" % (
                p, statistics.median(times[p]), min(times[p]), max(times[p]), int(np.isfinite(out[p]).sum()))
        if "simulate()" in paths:
            ok = np.isfinite(out["table"]) & np.isfinite(out["simulate()"])
            sim64 = statistics.median(times["simulate()"]) * 64.0 / N_SIM
            line += "\n  simulate() on %d candidates, scaled to 64: %.3f s | simulate() / table = %.1f | max relative score " \
                    "difference over %d scores %.2e" % (N_SIM, sim64, sim64 / statistics.median(times["table"]), int(ok.sum()),
                                                        float(np.max(np.abs(out["table"][ok] / out["simulate()"][ok] - 1)))
                                                        if ok.any() else float("nan"))
        print(line, flush=True)


TABLE = {"table": lambda b: table_ev.evaluate(b)}
measure("(a) Koopman", koopmans, dict(TABLE, **{"simulate()": by_simulate}), (64, 16, 1))
measure("(b) ARX", arxs, dict(TABLE, **{"in turn, own surrogate": own_surrogate_in_turn}), (64,))
measure("(b) ARX", arxs, TABLE, (16, 1))
mix = [m for pair in zip(arxs[:32], koopmans[:32]) for m in pair]
measure("(b) half ARX, half Koopman", mix, TABLE, (64,))


# ---- (c) the two kernels of an iteration --------------------------------------------------------------------------------
def stage(m, wide=None):
    h = _lib.Handle(0, "f64", jit=False)
    old = os.environ.pop("AMPC_LINEAR_WIDE", None)
    if wide:
        os.environ["AMPC_LINEAR_WIDE"] = "1"
    try:
        h.set_linear(m.A, m.B)
    finally:
        os.environ.pop("AMPC_LINEAR_WIDE", None)
        if old is not None:
            os.environ["AMPC_LINEAR_WIDE"] = old
    return h


def costs_on(h):
    P = len(cands)
    h.set_quad_costs(np.stack([np.diag(c["Q"]) for c in cands]), np.stack([np.diag(c["R"]) for c in cands]),
                     np.stack([np.diag(c["F"]) for c in cands]), np.zeros((P, NO)))
    h.set_ctrl_bounds(np.full(NU, -0.5), np.full(NU, 0.5))


def kernel_split(title, models, index, table=True, wide=None):
    """Mean sweep / line-search time per iteration of a 64-problem queue through 64 slots."""
    one_row = Trajectory(system, 1, np.array([[0.2, -0.1, 0.1, 0.0]]), np.zeros((1, NU)))
    H = max(c["horizon"] for c in cands)
    hz = np.array([c["horizon"] for c in cands], dtype=np.int32)
    if table:
        h = _lib.Handle(0, "f64", jit=False)
        h.set_linear(np.zeros((NO, NO)), np.zeros((NO, NU)))
    else:
        h = stage(models[0], wide)
    costs_on(h)
    plan = _lib.IlqrPlan(h, 64, H, system.dt, cost_index=np.arange(64), clip_to_bounds=True)
    handles = []
    if table:
        handles = [stage(m) for m in models]
        plan.set_linear_models(handles)
        x0 = [np.asarray(models[k].traj_to_state(one_row)) for k in index]
        kw = dict(model_index=np.asarray(index, dtype=np.int32))
    else:
        x0 = np.tile(np.asarray(models[0].traj_to_state(one_row)), (64, 1))
        kw = {}
    res = []
    for r in range(REPS + 1):
        plan.set_timing(True)
        out = plan.solve_queue(x0, None, np.arange(64), max_iter=50, gains=False, horizon=hz, **kw)
        tm = plan.timing()
        if r:
            res.append((tm["riccati_ms"], tm["iter_ms"]))
    sw, ls = [x[0] for x in res], [x[1] for x in res]
    print("%-58s sweep %.4f ms (min %.4f, max %.4f) | line search %.4f ms (min %.4f, max %.4f) per iteration | "
          "iterations %d..%d" % (title, statistics.median(sw), min(sw), max(sw), statistics.median(ls), min(ls), max(ls),
                                 int(out["iters"].min()), int(out["iters"].max())), flush=True)
    plan.close()
    for x in handles + [h]:
        x.close()


idx = [i % 64 for i in range(64)]
kernel_split("(c) table of the 64 ARX models (states <= %d)" % max(m.state_dim for m in arxs), arxs, idx)
wide128 = Koopman(system, poly_basis="true", poly_degree=2, trig_basis="true", trig_freq=15, strict_reference=False)
wide128.train(data, silent=True)                                                    # 4 * (1 + 1 + 30) = 128 states
assert wide128.state_dim == 128
kernel_split("(c) the same with one unused 128-state entry", arxs + [wide128], idx)
kernel_split("(c) the same, one problem on the 128-state entry", arxs + [wide128], idx[:63] + [64])
big = max(arxs, key=lambda m: m.state_dim)
kernel_split("(c) one-model table, %d states" % big.state_dim, [big], [0] * 64)
kernel_split("(c) single-model plan, staged wide", [big], None, table=False, wide=True)
kernel_split("(c) single-model plan, as ampc_set_linear stages it", [big], None, table=False)
kernel_split("(c) one-model table, 128 states", [wide128], [0] * 64)
kernel_split("(c) single-model plan, 128 states", [wide128], None, table=False)
