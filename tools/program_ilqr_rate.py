"""Perfect-model iLQR at CartPole shape (4 observations, 1 control, the task's 200 rows): the traced CartPole program
(sysid/program.py) as the controller model AND the simulation model -- ``IlqrCandidateEvaluator(system, task, prog_i,
surrogate=prog)`` with ``prog_i = prog.differentiable(ilqr=True)``, every candidate's episode in one device-resident
closed loop (csrc/ilqr_kernels.hpp DYN = 3, ilqr_program_jacobian_kernel) -- against the only way there was before it:
the oracle's numpy iLQR on the program's host ``pred_diff``, stepped in a host loop, one candidate after the other.

Candidates from the reference's ranges (random_ilqr_candidates: horizon 5-25), the first 64, 16 and 1 of them,
``max_iter`` 50.  For context the same batch with a 2 x 128 tanh MLP as the controller model (the program stays the
simulation model: tools/truedyn_rate.py's iLQR line).

Medians of `repetitions` alternating repetitions after one warm-up of each path; the host clock runs around calls that
end in a synchronise.  ``--host-reps K`` repeats the host path K times only (at 64 candidates one repetition is
minutes).  A host episode that ends in the reference's LinAlgError (a singular Quu) counts as not finite, as the
device's status 1 does.
python tools/program_ilqr_rate.py [repetitions] [--host-reps K]"""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import DynamicsProgram, QuadCost, System, Task      # noqa: E402
from autompc_amd.tuning import IlqrCandidateEvaluator, random_ilqr_candidates      # noqa: E402
from oracle.costs import QuadCostOracle      # noqa: E402
from oracle.ilqr import ILQROracle      # noqa: E402
from truedyn_rate import DT, STEPS, cartpole, controller_model      # noqa: E402

ARGV = sys.argv[1:]
HOST_REPS = None
if "--host-reps" in ARGV:
    k = ARGV.index("--host-reps")
    HOST_REPS = max(1, int(ARGV[k + 1]))
    del ARGV[k:k + 2]
REPS = max(1, int(ARGV[0])) if ARGV else 5
HOST_REPS = min(3, REPS) if HOST_REPS is None else min(HOST_REPS, REPS)
UMAX = 20.0
INIT = np.array([3.1, 0.0, 0.0, 0.0])
MAX_ITER = 50


def host_episode(prog_d, c):
    """One candidate's episode with the numpy iLQR planning on the program's host Jacobians and the program as the
    dynamics; the last observation is returned so that nothing is optimised away (NaN after a singular Quu)."""
    orc = ILQROracle(prog_d, QuadCostOracle(np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), np.zeros(4)), DT,
                     int(c["horizon"]), ubounds=(np.array([-UMAX]), np.array([UMAX])), max_iter=MAX_ITER)
    x, cs = INIT.copy(), np.concatenate([INIT, np.zeros(1)])
    try:
        for _ in range(STEPS - 1):
            u, cs = orc.run(cs, x)
            x = prog_d.pred(x, u)
    except (np.linalg.LinAlgError, UnboundLocalError):
        return np.full(4, np.nan)
    return x


def main():
    system = System(["theta", "omega", "x", "dx"], ["u"], dt=DT)
    task = Task(system)
    task.set_cost(QuadCost(system, np.eye(4), 0.01 * np.eye(1), np.eye(4)))
    task.set_ctrl_bounds([-UMAX], [UMAX])
    task.set_init_obs(INIT)
    task.set_num_steps(STEPS)
    prog = DynamicsProgram.trace(system, cartpole)
    prog_i = prog.differentiable(ilqr=True)
    print("program: %d instructions, %d slots (JVP: %d, %d); %d rows per episode; max_iter %d; %d repetitions (host "
          "path: %d)" % (prog.code.shape[0], prog.n_slots, prog_i.jvp.code.shape[0], prog_i.jvp.n_slots, STEPS, MAX_ITER,
                         REPS, HOST_REPS), flush=True)
    on_prog = IlqrCandidateEvaluator(system, task, prog_i, surrogate=prog)
    on_mlp = IlqrCandidateEvaluator(system, task, controller_model(system), surrogate=prog)
    cands = random_ilqr_candidates(system, 64, seed=0)
    on_prog.evaluate(cands[:1], max_iter=MAX_ITER)               # warm-up: plans, kernels
    on_mlp.evaluate(cands[:1], max_iter=MAX_ITER)
    host_episode(prog_i, dict(cands[0], horizon=5))
    for B in (64, 16, 1):
        batch = cands[:B]
        on_prog.evaluate(batch, max_iter=MAX_ITER)
        on_mlp.evaluate(batch, max_iter=MAX_ITER)
        dev, mlp, host = [], [], []
        for r in range(REPS):
            t0 = time.perf_counter()
            sc = on_prog.evaluate(batch, max_iter=MAX_ITER)
            dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            on_mlp.evaluate(batch, max_iter=MAX_ITER)
            mlp.append(time.perf_counter() - t0)
            if r < HOST_REPS:
                t0 = time.perf_counter()
                last = [host_episode(prog_i, c) for c in batch]
                host.append(time.perf_counter() - t0)
        d, m, h = (1e3 * statistics.median(v) for v in (dev, mlp, host))
        print("iLQR %2d candidates x %d rows: program as controller model %9.1f ms   numpy iLQR on the program in turn "
              "%11.1f ms   ratio %7.1fx   |   2 x 128 MLP as controller model %9.1f ms   (finite: %d / %d device, "
              "%d / %d host)" % (B, STEPS, d, h, h / d, m, int(np.isfinite(sc).sum()), B,
                                 int(np.all(np.isfinite(last), axis=1).sum()), B), flush=True)


if __name__ == "__main__":
    main()
