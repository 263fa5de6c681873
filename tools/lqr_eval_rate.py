"""LqrCandidateEvaluator on HalfCheetah-shaped candidates (17 observations, 6 controls) against a seeded 2 x 256 MLP
surrogate: candidates/s for 64 and 256 candidates on ARX history 4 (91 states), history 10 (235 states) and an
ARX / Koopman mix, split into the gain launch and the closed loop, and the host simulate() loop over drop-in LQR
controllers for a few candidates.  python tools/lqr_eval_rate.py [n_steps]"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import ARX, MLP, Koopman, QuadCost, System, Task, Trajectory, simulate   # noqa: E402
from autompc_amd import _lib                                                              # noqa: E402
from autompc_amd.control.lqr import LQR                                                   # noqa: E402
from autompc_amd.tuning import LqrCandidateEvaluator                                      # noqa: E402
from oracle import mlp as omlp                                                            # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 200
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


def candidates(n, models, seed):
    rng = np.random.default_rng(seed)
    return [{"controller": "lqr", "finite_horizon": True, "horizon": int(rng.integers(1, 1001)),
             "model": models[i % len(models)], "Q": 10 ** rng.uniform(-1, 1, NO), "R": 10 ** rng.uniform(-1, 1, NU),
             "F": 10 ** rng.uniform(-1, 1, NO)} for i in range(n)]


def gains_only(cands):
    """The evaluator's gain launch alone (staging and uploads included)."""
    hs = {id(c["model"]): c["model"]._dev() for c in cands}
    plan = _lib.LqrPlan([hs[id(c["model"])] for c in cands], NO, NU)
    t0 = time.perf_counter()
    plan.gains([c["horizon"] for c in cands], np.array([np.diag(c["Q"]) for c in cands]),
               np.array([np.diag(c["R"]) for c in cands]), np.array([np.diag(c["F"]) for c in cands]))
    dt = time.perf_counter() - t0
    plan.close()
    return dt


ev = LqrCandidateEvaluator(s, task, surrogate=sur)
ev.evaluate(candidates(2, [arx4, koop], 99))                 # warm-up: library load, first launches
print("closed loop: %d control steps against a 2 x 256 relu MLP surrogate; horizons uniform in 1..1000" % (T - 1))
for name, models in (("ARX h4 (91 states)", [arx4]), ("ARX h10 (235 states)", [arx10]),
                     ("mix ARX h4 / h10 / Koopman (153)", [arx4, arx10, koop])):
    for n in (64, 256):
        cands = candidates(n, models, n)
        tg = gains_only(cands)
        t0 = time.perf_counter()
        sc = ev.evaluate(cands)
        dt = time.perf_counter() - t0
        print("%-34s %4d candidates: %.3f s = %7.1f candidates/s  (gains %.3f s, closed loop + staging %.3f s; "
              "finite %d)" % (name, n, dt, n / dt, tg, dt - tg, int(np.isfinite(sc).sum())))
# the host loop: simulate() over drop-in controllers (gain on the device, run() and the surrogate step per call)
k = 4
cands = candidates(k, [arx4, arx10, koop], 7)
t0 = time.perf_counter()
for c in cands:
    t = Task(s)
    t.set_cost(QuadCost(s, np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"])))
    t.set_ctrl_bounds(-np.ones(NU), np.ones(NU))
    ctl = LQR(s, t, c["model"], "true", c["horizon"])
    ctl.reset()
    task.get_cost()(simulate(ctl, task.get_init_obs(), task.term_cond, sim_model=sur, max_steps=T))
dt = time.perf_counter() - t0
print("host simulate() over drop-in LQR, %d candidates: %.3f s = %.1f candidates/s" % (k, dt, k / dt))
