"""Perfect-model MPPI at CartPole shape (4 observations, 1 control, the task's 200 rows): the traced CartPole program
(sysid/program.py) as the controller model AND the simulation model -- ``CandidateEvaluator(system, task, prog_d,
surrogate=prog)``, every candidate's episode in one device-resident closed loop on mppi_rollout_program_kernel --
against the only way there was before it: the oracle's numpy MPPI with the program's host evaluation as
``pred_batch``, stepped in a host loop, one candidate after the other.

Candidates from the reference's ranges (random_candidates: horizon 5-30, num_path 100-1000), the first 64, 16 and 1 of
them.  For context the same batch with a 2 x 128 tanh MLP as the controller model (the program stays the simulation
model: tools/truedyn_rate.py's MPPI line).

Medians of `repetitions` alternating repetitions after one warm-up of each path; the host clock runs around calls that
end in a synchronise.  ``--host-reps K`` repeats the host path K times only (at 64 candidates one repetition is
minutes).
python tools/program_mppi_rate.py [repetitions] [--host-reps K]"""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import DynamicsProgram, QuadCost, System, Task      # noqa: E402
from autompc_amd.tuning import CandidateEvaluator, random_candidates      # noqa: E402
from oracle.costs import QuadCostOracle      # noqa: E402
from oracle.mppi import MPPIOracle      # noqa: E402
from truedyn_rate import DT, STEPS, cartpole, controller_model      # noqa: E402

ARGV = sys.argv[1:]
HOST_REPS = None
if "--host-reps" in ARGV:
    k = ARGV.index("--host-reps")
    HOST_REPS = max(1, int(ARGV[k + 1]))
    del ARGV[k:k + 2]
REPS = max(1, int(ARGV[0])) if ARGV else 5
HOST_REPS = REPS if HOST_REPS is None else min(HOST_REPS, REPS)
UMAX = 20.0
INIT = np.array([3.1, 0.0, 0.0, 0.0])


def host_episode(prog, c, seed):
    """One candidate's episode with the numpy MPPI planning on the program and the program as the dynamics: the score
    is not needed here, the last observation is returned so that nothing is optimised away."""
    np.random.seed(seed)
    orc = MPPIOracle(prog, QuadCostOracle(np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), np.zeros(4)),
                     np.array([[-UMAX, UMAX]]), horizon=int(c["horizon"]), num_path=int(c["num_path"]),
                     sigma=float(c["sigma"]), lmda=float(c["lmda"]))
    x, cs = INIT.copy(), np.concatenate([INIT, np.zeros(1)])
    for _ in range(STEPS - 1):
        u, cs = orc.run(cs, x)
        x = prog.pred(x, u)
    return x


def main():
    system = System(["theta", "omega", "x", "dx"], ["u"], dt=DT)
    task = Task(system)
    task.set_cost(QuadCost(system, np.eye(4), 0.01 * np.eye(1), np.eye(4)))
    task.set_ctrl_bounds([-UMAX], [UMAX])
    task.set_init_obs(INIT)
    task.set_num_steps(STEPS)
    prog = DynamicsProgram.trace(system, cartpole)
    prog_d = prog.differentiable()
    print("program: %d instructions, %d slots (JVP: %d, %d); %d rows per episode; %d repetitions (host path: %d)"
          % (prog.code.shape[0], prog.n_slots, prog_d.jvp.code.shape[0], prog_d.jvp.n_slots, STEPS, REPS, HOST_REPS),
          flush=True)
    on_prog = CandidateEvaluator(system, task, prog_d, surrogate=prog)
    on_mlp = CandidateEvaluator(system, task, controller_model(system), surrogate=prog)
    cands = random_candidates(system, 64, seed=0)
    on_prog.evaluate(cands[:1], seed=0)                          # warm-up: plans, kernels
    on_mlp.evaluate(cands[:1], seed=0)
    host_episode(prog, dict(cands[0], horizon=5, num_path=100), 0)
    for B in (64, 16, 1):
        batch = cands[:B]
        on_prog.evaluate(batch, seed=0)
        on_mlp.evaluate(batch, seed=0)
        dev, mlp, host = [], [], []
        for r in range(REPS):
            t0 = time.perf_counter()
            sc = on_prog.evaluate(batch, seed=0, index_offset=0)
            dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            on_mlp.evaluate(batch, seed=0, index_offset=0)
            mlp.append(time.perf_counter() - t0)
            if r < HOST_REPS:
                t0 = time.perf_counter()
                last = [host_episode(prog, c, i) for i, c in enumerate(batch)]
                host.append(time.perf_counter() - t0)
        d, m, h = (1e3 * statistics.median(v) for v in (dev, mlp, host))
        print("MPPI %2d candidates x %d rows: program as controller model %9.1f ms   numpy MPPI on the program in turn "
              "%11.1f ms   ratio %7.1fx   |   2 x 128 MLP as controller model %9.1f ms   (finite: %d / %d device, "
              "%d / %d host)" % (B, STEPS, d, h, h / d, m, int(np.isfinite(sc).sum()), B,
                                 int(np.all(np.isfinite(last), axis=1).sum()), B), flush=True)


if __name__ == "__main__":
    main()
