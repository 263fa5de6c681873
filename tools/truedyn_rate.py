"""The true-dynamics column of the tuner at CartPole shape (4 observations, 1 control, the task's 200 rows): a traced
CartPole program (sysid/program.py) as the simulation model of a second evaluator -- every candidate's episode in one
device-resident closed loop, ``BatchPipelineTuner(truedyn_evaluator=...)`` -- against the only way there was before it:
``BatchPipelineTuner.truedyn_score`` per candidate in turn, the drop-in controller under ``simulate()`` with the
dynamics as a host callback between solves.

  MPPI   candidates from the reference's ranges (random_candidates: horizon 5-30, num_path 100-1000)
  iLQR   candidates from the reference's ranges (random_ilqr_candidates: horizon 5-25)

for the first 64, 16 and 1 of them, on a 2 x 128 tanh MLP as the controllers' model.  Also: the device rollout of
500 x 200 trajectories (``uniform_random_generate(..., device=True)``: one ampc_program_rollout launch) against the
generator's host loop on the plain Python dynamics.

Medians of `repetitions` alternating repetitions after one warm-up of each path (the host path warms up on one
candidate); the host clock runs around calls that end in a synchronise.  ``--host-reps K`` repeats the per-candidate
host path K times only (at 64 iLQR candidates one repetition is minutes).
python tools/truedyn_rate.py [repetitions] [--host-reps K]"""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import MLP, DynamicsProgram, QuadCost, System, Task, data_generation      # noqa: E402
from autompc_amd.tuning import (BatchPipelineTuner, CandidateEvaluator, IlqrCandidateEvaluator,   # noqa: E402
                                random_candidates, random_ilqr_candidates)

ARGV = sys.argv[1:]
HOST_REPS = None
if "--host-reps" in ARGV:
    k = ARGV.index("--host-reps")
    HOST_REPS = max(1, int(ARGV[k + 1]))
    del ARGV[k:k + 2]
REPS = max(1, int(ARGV[0])) if ARGV else 5
HOST_REPS = REPS if HOST_REPS is None else min(HOST_REPS, REPS)
DT, STEPS = 0.05, 200


def cartpole(y, u, dt=DT, g=9.8, m=1.0, L=1.0, b=1.0):
    """The benchmark's form: Euler step of the simplified cart-pole, returns a fresh array."""
    theta, omega, x, dx = y
    return np.array([theta + dt * omega,
                     omega + dt * (g * np.sin(theta) / L - b * omega / (m * L ** 2) + u[0] * np.cos(theta) / L),
                     x + dt * dx,
                     dx + dt * u[0]])


def controller_model(system, seed=0, hidden=128):
    rng = np.random.default_rng(seed)
    sizes = [5, hidden, hidden, 4]
    m = MLP(system, n_hidden_layers=2, hidden_size_1=hidden, hidden_size_2=hidden, nonlintype="tanh")
    m.weights = [rng.normal(scale=0.5 / np.sqrt(sizes[i]), size=(sizes[i + 1], sizes[i])) for i in range(3)]
    m.biases = [rng.normal(scale=0.05, size=sizes[i + 1]) for i in range(3)]
    m.xu_means, m.xu_std = np.zeros(5), np.array([3.0, 5.0, 3.0, 5.0, 10.0])
    m.dy_means, m.dy_std = np.zeros(4), np.array([0.2, 1.0, 0.2, 1.0])
    return m


def median_ms(samples):
    return 1e3 * statistics.median(samples)


def main():
    system = System(["theta", "omega", "x", "dx"], ["u"], dt=DT)
    task = Task(system)
    task.set_cost(QuadCost(system, np.eye(4), 0.01 * np.eye(1), np.eye(4)))
    task.set_ctrl_bounds([-20.0], [20.0])
    task.set_init_obs(np.array([3.1, 0.0, 0.0, 0.0]))
    task.set_num_steps(STEPS)
    prog = DynamicsProgram.trace(system, cartpole)
    model = controller_model(system)
    print("program: %d instructions, %d slots; %d rows per episode; %d repetitions (host path: %d)"
          % (prog.code.shape[0], prog.n_slots, STEPS, REPS, HOST_REPS), flush=True)
    for name, Ev, draw in (("MPPI", CandidateEvaluator, random_candidates),
                           ("iLQR", IlqrCandidateEvaluator, random_ilqr_candidates)):
        ev = Ev(system, task, model)
        true = Ev(system, task, model, surrogate=prog)
        tuner = BatchPipelineTuner(system, ev, truedyn_evaluator=true)
        cands = draw(system, 64, seed=0)
        true.evaluate(cands[:1], seed=0)                         # warm-up: plans, kernels
        tuner.truedyn_score(cands[0], cartpole, seed=0)
        for B in (64, 16, 1):
            batch = cands[:B]
            true.evaluate(batch, seed=0)
            dev, host = [], []
            for r in range(REPS):
                t0 = time.perf_counter()
                sc = true.evaluate(batch, seed=0, index_offset=0)
                dev.append(time.perf_counter() - t0)
                if r < HOST_REPS:
                    t0 = time.perf_counter()
                    hs = [tuner.truedyn_score(c, cartpole, seed=i) for i, c in enumerate(batch)]
                    host.append(time.perf_counter() - t0)
            d, h = median_ms(dev), median_ms(host)
            print("%s %2d candidates x %d rows: truedyn_evaluator %9.1f ms   truedyn_score in turn %10.1f ms   "
                  "ratio %6.1fx   (finite scores: %d / %d device, %d / %d host)"
                  % (name, B, STEPS, d, h, h / d, int(np.isfinite(sc).sum()), B, int(np.isfinite(hs).sum()), B),
                  flush=True)
    # data generation: 500 trajectories x 200 rows
    lo, hi = [-3.2, -1.0, -1.0, -1.0], [3.2, 1.0, 1.0, 1.0]

    def gen(dynamics, **kw):
        return data_generation.uniform_random_generate(system, task, dynamics, np.random.default_rng(0), lo, hi, STEPS,
                                                       500, **kw)
    a, b = gen(prog, device=True), gen(cartpole)
    worst = max(float(np.max(np.abs(x.obs - y.obs))) for x, y in zip(a, b))
    dev, host = [], []
    for r in range(REPS):
        t0 = time.perf_counter()
        gen(prog, device=True)
        dev.append(time.perf_counter() - t0)
        if r < HOST_REPS:
            t0 = time.perf_counter()
            gen(cartpole)
            host.append(time.perf_counter() - t0)
    d, h = median_ms(dev), median_ms(host)
    print("uniform_random_generate 500 x %d rows: device rollout %8.1f ms   host loop %9.1f ms   ratio %5.1fx   "
          "(largest difference of an observation: %.2e)" % (STEPS, d, h, h / d, worst), flush=True)
    x0 = np.random.default_rng(1).uniform(lo, hi, (500, 4))
    U = np.random.default_rng(2).uniform(-20, 20, (500, STEPS, 1))
    prog.rollout(x0, U, device=True)
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        prog.rollout(x0, U, device=True)
        t.append(time.perf_counter() - t0)
    print("ampc_program_rollout 500 x %d steps alone (upload, launch, download): %.2f ms" % (STEPS, median_ms(t)),
          flush=True)


if __name__ == "__main__":
    main()
