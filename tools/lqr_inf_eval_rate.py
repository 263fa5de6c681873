"""LqrCandidateEvaluator(infinite_horizon="iterate") on the mixes of tools/lqr_eval_rate.py (17 observations, 6
controls, a seeded 2 x 256 MLP surrogate) with every other candidate infinite: time and candidates/s next to the same
mix with every candidate finite, the distribution of the Riccati step counts, and the host alternative for a few
infinite candidates (lqr_gain_inf_host + simulate()).  python tools/lqr_inf_eval_rate.py [n_steps] [inf_max_iter]"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import ARX, MLP, Koopman, QuadCost, System, Task, Trajectory, simulate   # noqa: E402
from autompc_amd.control.lqr import RiccatiNotConverged                                   # noqa: E402
from autompc_amd.tuning import LqrCandidateEvaluator                                      # noqa: E402
from autompc_amd.tuning.lqr_eval import _HostInfiniteHorizonLQR                           # noqa: E402
from oracle import mlp as omlp                                                            # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 200
MAX_ITER = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
NO, NU = 17, 6
s = System(["x%d" % i for i in range(NO)], ["u%d" % i for i in range(NU)], dt=0.05)


def trajs(seed, n=8, L=120):
    rng = np.random.default_rng(seed)
    A = 0.9 * np.linalg.qr(rng.normal(size=(NO, NO)))[0]
    B = 0.3 * rng.normal(size=(NO, NU))
    out = []
    for _ in range(n):
        obs, ctl = np.zeros((L, NO)), rng.normal(size=(L, NU))
        x = rng.normal(size=NO)
        for i in range(L):
            obs[i] = x
            x = A @ x + B @ ctl[i] + 0.01 * rng.normal(size=NO)
        out.append(Trajectory(s, L, obs, ctl))
    return out


data = trajs(1)
arx4, arx10 = ARX(s, history=4), ARX(s, history=10)
arx4.train(data)
arx10.train(data)
koop = Koopman(s, method="lstsq", poly_basis=True, poly_degree=3, trig_basis=True)      # 9 functions: 153 states
koop.train(data)
p = omlp.random_params(NO, NU, [256, 256], "relu", seed=7)
sur = MLP(s, n_hidden_layers=2, hidden_size=256, nonlintype="relu")
sur.weights, sur.biases = p["weights"], p["biases"]
sur.xu_means, sur.xu_std, sur.dy_means, sur.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
task = Task(s)
task.set_cost(QuadCost(s, np.eye(NO), 0.01 * np.eye(NU), np.eye(NO)))
task.set_ctrl_bounds(-np.ones(NU), np.ones(NU))
task.set_init_obs(np.random.default_rng(0).uniform(-0.1, 0.1, NO))
task.set_num_steps(T)


def candidates(n, models, seed, half_infinite):
    """lqr_eval_rate.py's candidates; with half_infinite every odd one becomes an infinite horizon."""
    rng = np.random.default_rng(seed)
    out = [{"controller": "lqr", "finite_horizon": True, "horizon": int(rng.integers(1, 1001)),
            "model": models[i % len(models)], "Q": 10 ** rng.uniform(-1, 1, NO), "R": 10 ** rng.uniform(-1, 1, NU),
            "F": 10 ** rng.uniform(-1, 1, NO)} for i in range(n)]
    if half_infinite:
        for c in out[1::2]:
            c["finite_horizon"] = False
    return out


ev = LqrCandidateEvaluator(s, task, surrogate=sur, infinite_horizon="iterate", inf_max_iter=MAX_ITER)
ev.evaluate(candidates(2, [arx4, koop], 99, True))             # warm-up: library load, first launches
print("closed loop: %d control steps against a 2 x 256 relu MLP surrogate; finite horizons uniform in 1..1000; "
      "threshold 1e-3, at most %d Riccati steps" % (T - 1, MAX_ITER))
for name, models in (("ARX h4 (91 states)", [arx4]), ("ARX h10 (235 states)", [arx10]),
                     ("mix ARX h4 / h10 / Koopman (153)", [arx4, arx10, koop])):
    for n in (64, 256):
        row = []
        for half in (False, True):
            cands = candidates(n, models, n, half)
            t0 = time.perf_counter()
            sc = ev.evaluate(cands)
            row.append(time.perf_counter() - t0)
        inf = np.array([not c["finite_horizon"] for c in cands])
        it, st = ev.last_iterations[inf], ev.last_status[inf]
        q = np.percentile(it[st == 0], [0, 50, 90, 100]).astype(int) if np.any(st == 0) else [0] * 4
        print("%-34s %4d candidates: all finite %.3f s = %7.1f candidates/s; half infinite %.3f s = %7.1f candidates/s; "
              "Riccati steps of the %d converged: min %d, median %d, 90 %% %d, max %d; not converged %d; singular %d"
              % (name, n, row[0], n / row[0], row[1], n / row[1], int((st == 0).sum()), q[0], q[1], q[2], q[3],
                 int((st == 3).sum()), int((st == 1).sum())))
# the host alternative: the drop-in with the host iteration under simulate(), a few infinite candidates of the mix
k = 4
cands = [c for c in candidates(16, [arx4, arx10, koop], 7, True) if not c["finite_horizon"]][:k]
t0 = time.perf_counter()
done = 0
for c in cands:
    t = Task(s)
    t.set_cost(QuadCost(s, np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"])))
    t.set_ctrl_bounds(-np.ones(NU), np.ones(NU))
    try:
        ctl = _HostInfiniteHorizonLQR(s, t, c["model"], "iterate", 1e-3, MAX_ITER)
    except RiccatiNotConverged:
        continue
    ctl.reset()
    task.get_cost()(simulate(ctl, task.get_init_obs(), task.term_cond, sim_model=sur, max_steps=T))
    done += 1
dt = time.perf_counter() - t0
print("host lqr_gain_inf_host + simulate(), %d infinite candidates (%d converged): %.3f s = %.1f candidates/s"
      % (k, done, dt, k / dt))
