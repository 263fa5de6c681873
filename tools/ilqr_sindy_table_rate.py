"""IlqrCandidateEvaluator(sindy_models="table") (ONE iLQR plan with a table of SINDy models of any mix of feature
libraries: the line search and the Jacobians of csrc/ilqr_sindy_table_kernels.hpp) against the only way there was before
it: one IlqrCandidateEvaluator per model, each evaluating the candidates that carry its model -- in turn, and side by
side on 8 host threads -- for 64 iLQR candidates (random_ilqr_candidates) x 49 control steps at CartPole shape (4
observations, 1 control), max_iter 50.  The controller models are 64 configurations drawn from SINDyFactory's ranges by
default_rng(0) (draws over the device fit's feature cap are drawn again), fitted once by fit_sindy_models on 100
trajectories x 200 rows; a batch uses the first 64, 16 or 1 of them.  The three paths alternate in one process after one
warm-up each; the host clock runs around evaluate(), which ends in a synchronise.
python tools/ilqr_sindy_table_rate.py [repetitions] [--table-only]
  --table-only: the 64-model table path alone, the run rocprofv3 --kernel-trace --stats traces."""
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import QuadCost, SINDy, System, Task, Trajectory        # noqa: E402
from autompc_amd.sysid.sindy_fit import MAX_FEATURES, fit_sindy_models   # noqa: E402
from autompc_amd.tuning import IlqrCandidateEvaluator, random_ilqr_candidates   # noqa: E402
from autompc_amd.tuning.batch_eval import candidate_models               # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = max(5, int(ARGS[0])) if ARGS else 5
TABLE_ONLY = "--table-only" in sys.argv
N_MODELS, NO, NU = 64, 4, 1


def trajs(s, seed, n=100, L=200):
    """A damped nonlinear oscillator driven by random controls, scaled to |x| <= 0.8 (tools/sindy_fit_rate.py)."""
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


def sample_config(rng):
    """One draw from SINDyFactory's space (sysid/sindy.py: get_configuration_space)."""
    kw = dict(time_mode=str(rng.choice(["discrete", "continuous"])), poly_basis=bool(rng.integers(2)),
              trig_basis=bool(rng.integers(2)), threshold=float(10.0 ** rng.uniform(-5.0, 1.0)))
    if kw["poly_basis"]:
        kw.update(poly_degree=int(rng.integers(2, 9)), poly_cross_terms=bool(rng.integers(2)))
    if kw["trig_basis"]:
        kw.update(trig_freq=int(rng.integers(1, 9)), trig_interaction=bool(rng.integers(2)))
    return kw


system = System(["x%d" % i for i in range(NO)], ["u%d" % i for i in range(NU)], dt=0.05)
data = trajs(system, 1)
rng = np.random.default_rng(0)
kws, redrawn = [], 0
while len(kws) < N_MODELS:
    kw = sample_config(rng)
    if len(SINDy(system, **kw).library[0]) <= MAX_FEATURES:
        kws.append(kw)
    else:
        redrawn += 1
models = [SINDy(system, **kw) for kw in kws]
t0 = time.perf_counter()
rep = fit_sindy_models(models, data)
feats = [m.coefficients.shape[1] for m in models]
print("%d SINDy configurations fitted in %.2f s (device fits %d, host fits %d; %d draws over %d features drawn again): "
      "%d distinct libraries, %d .. %d features, %d continuous"
      % (len(models), time.perf_counter() - t0, rep.device_fits, rep.host_fits, redrawn, MAX_FEATURES,
         len({(m.coefficients.shape[1], m.time_mode, m.trig_freq, m.poly_degree) for m in models}), min(feats), max(feats),
         sum(m.time_mode == "continuous" for m in models)), flush=True)

task = Task(system)
task.set_cost(QuadCost(system, np.eye(NO), 0.01 * np.eye(NU), np.eye(NO)))
task.set_ctrl_bounds(np.full(NU, -0.5), np.full(NU, 0.5))
task.set_init_obs(np.array([0.2, -0.1, 0.1, 0.0]))
task.set_num_steps(50)
surrogate = next(m for m in models if m.time_mode == "discrete")
cands = random_ilqr_candidates(system, 64, seed=0)
for c in cands:
    c["Q"], c["R"], c["F"] = c["Q"] ** 0.25, c["R"] ** 0.25, c["F"] ** 0.25
table_ev = IlqrCandidateEvaluator(system, task, surrogate, sindy_models="table")
MAX_ITER = 50


def per_model(batch, threads):
    """The path before the table: one evaluator per model object, on the candidates that carry it."""
    ms, index = candidate_models(batch, surrogate)
    scores = np.empty(len(batch))

    def one(k):
        ids = np.nonzero(index == k)[0]
        ev = IlqrCandidateEvaluator(system, task, ms[k], surrogate=surrogate)
        scores[ids] = ev.evaluate([{key: v for key, v in batch[i].items() if key != "model"} for i in ids],
                                  max_iter=MAX_ITER)
    if threads > 1:
        with ThreadPoolExecutor(max_workers=threads) as pool:
            list(pool.map(one, range(len(ms))))
    else:
        for k in range(len(ms)):
            one(k)
    return scores


PATHS = {"table": lambda b: table_ev.evaluate(b, max_iter=MAX_ITER)}
if not TABLE_ONLY:
    PATHS["in turn"] = lambda b: per_model(b, 1)
    PATHS["8 threads"] = lambda b: per_model(b, 8)

for n_models in ((64,) if TABLE_ONLY else (64, 16, 1)):
    batch = [dict(c, model=models[i % n_models]) for i, c in enumerate(cands)]
    out, times = {}, {p: [] for p in PATHS}
    for p, run in PATHS.items():                                       # warm-up: kernels loaded, allocator primed
        run(batch)
    for _ in range(REPS):
        for p, run in PATHS.items():
            t0 = time.perf_counter()
            out[p] = run(batch)
            times[p].append(time.perf_counter() - t0)
    assert table_ev.last_models == {"path": "sindy_table", "models": n_models, "plans": 1}, table_ev.last_models
    line = "%2d models, 64 candidates x 49 control steps, %d repetitions:" % (n_models, REPS)
    for p in PATHS:
        line += "\n  %-9s median %.4f s (min %.4f, max %.4f) | finite scores %d" % (
            p, statistics.median(times[p]), min(times[p]), max(times[p]), int(np.isfinite(out[p]).sum()))
    if not TABLE_ONLY:
        ok = np.isfinite(out["table"]) & np.isfinite(out["in turn"])
        line += "\n  in turn / table = %.2f | 8 threads / table = %.2f | max relative score difference over the %d finite " \
                "scores %.2e" % (statistics.median(times["in turn"]) / statistics.median(times["table"]),
                                 statistics.median(times["8 threads"]) / statistics.median(times["table"]), int(ok.sum()),
                                 float(np.max(np.abs(out["table"][ok] / out["in turn"][ok] - 1))) if ok.any() else
                                 float("nan"))
    print(line, flush=True)
