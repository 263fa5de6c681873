"""Shared by the tests of the MPPI plan that holds a table of linear models of mixed state dimension
(ampc_mppi_plan_set_linear_models, csrc/mppi_linear_table_kernels.hpp): four sets of synthetic models x' = A x + B u and
for every set ONE fixed plan -- problems, control bounds (-1, 1), cost blocks, initial states, warm starts and noise.

  edges  3 observations / 2 controls  nx 3, 9, 15, 16, 17: k-steps 2, 3, 5, 5, 5 (the k-loop's remainder) and one or two
                                      column tiles (the first tile boundary)
  wide   3 / 2                        nx 62, 64, 65, 130, 256: the staging boundary of ampc_set_linear, a wave that owns
                                      two column tiles (more than eight tiles), the maximum
  k4     3 / 2                        nx 6, 14: k-steps 2 and 4 -- the unrolled k-loop with no remainder
  nu6    5 / 6                        nx 5, 23, 70

A = 0.9 Q + small noise with Q orthogonal (spectral radius < 1) keeps every rollout finite.  Sample counts sit on the
16-sample tile (1, 4, 5, 63, 64, 65, 130); horizons are 2 (the smallest a plan takes), 3, 5 and the cap of 8;
model_index is non-monotonic and the LAST table entry of every set is used by no problem.  cpu_rollouts() is the oracle's
MPPI in numpy: tests/test_mppi_linear_table_host.py checks on the CPU that every cost is finite, the precondition of the
bitwise GPU tests."""
import functools

import numpy as np

from helpers import make_system

HORIZON_CAP = 8
N_LIST = (1, 4, 5, 63, 64, 65, 130)
H_LIST = (2, 8, 3, 2, 8, 5, 8)
SIGMA, LMDA = 0.3, 0.7
LO, HI = -1.0, 1.0
# (obs_dim, nu, state dimensions of the table, model of each problem); the last entry is a spare nobody uses
SETS = {
    "edges": dict(no=3, nu=2, nx=(3, 9, 15, 16, 17, 7), index=(4, 0, 3, 1, 2, 4, 0)),
    "wide": dict(no=3, nu=2, nx=(62, 64, 65, 130, 256, 40), index=(2, 4, 0, 3, 1, 4, 3)),
    "k4": dict(no=3, nu=2, nx=(6, 14, 5), index=(1, 0, 1, 1, 0, 0, 1)),
    "nu6": dict(no=5, nu=6, nx=(5, 23, 70, 11), index=(2, 0, 1, 2, 1, 0, 2)),
}


def ksn(nx, nu):
    """k-steps of four of the MFMA rollout: ceil((nx + nu) / 4)."""
    return (nx + nu + 3) // 4


@functools.lru_cache(maxsize=None)
def matrices(name):
    """(system, [(A, B) ...]) of a set.  Read-only."""
    s = SETS[name]
    out = []
    for k, nx in enumerate(s["nx"]):
        rng = np.random.default_rng(1000 * len(name) + 10 * k + nx)
        A = 0.9 * np.linalg.qr(rng.normal(size=(nx, nx)))[0] + 0.02 * rng.normal(size=(nx, nx)) / np.sqrt(nx)
        assert np.max(np.abs(np.linalg.eigvals(A))) < 1.0
        B = rng.normal(scale=0.3, size=(nx, s["nu"]))
        A.setflags(write=False)
        B.setflags(write=False)
        out.append((A, B))
    return make_system(s["no"], s["nu"]), out


@functools.lru_cache(maxsize=None)
def plan_data(name):
    """The set's plan: per problem N, H, model index, x0 (its model's state dimension), warm start [H][nu], noise
    [N][H][nu], diagonal Q / R / F and a goal.  Read-only: the tests share it."""
    s = SETS[name]
    no, nu = s["no"], s["nu"]
    rng = np.random.default_rng({"edges": 51, "wide": 52, "k4": 53, "nu6": 54}[name])
    B = len(N_LIST)
    d = dict(N=np.array(N_LIST, dtype=np.int32), H=np.array(H_LIST, dtype=np.int32),
             index=np.array(s["index"], dtype=np.int32),
             x0=[rng.uniform(-0.3, 0.3, size=s["nx"][k]) for k in s["index"]],
             act=[rng.normal(scale=0.4, size=(int(h), nu)) for h in H_LIST],
             eps=[rng.normal(scale=np.sqrt(SIGMA), size=(int(n), int(h), nu)) for n, h in zip(N_LIST, H_LIST)],
             Q=np.stack([np.diag(rng.uniform(0.5, 2.0, no)) for _ in range(B)]),
             R=np.stack([np.diag(rng.uniform(0.01, 0.1, nu)) for _ in range(B)]),
             F=np.stack([np.diag(rng.uniform(0.5, 2.0, no)) for _ in range(B)]),
             goal=rng.normal(scale=0.1, size=(B, no)))
    for v in d.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return d


def indicator_terms(name):
    """A threshold and a box term on the observation (autompc_amd.costs.cost_terms layout, kinds 1 / 2), placed so that
    some rollouts violate them and others do not."""
    from autompc_amd import BoxThresholdCost, ThresholdCost
    from autompc_amd.costs.blocks import mppi_cost_parts
    system = matrices(name)[0]
    no = system.obs_dim
    limits = np.tile([-0.3, 0.35], (no, 1))
    limits[0, 0], limits[no - 1, 1] = -np.inf, np.inf
    cost = ThresholdCost(system, np.zeros(no), [0, 2], 0.25) + BoxThresholdCost(system, limits)
    return mppi_cost_parts(cost, no, system.ctrl_dim)[1]


class LinearOracle:
    """x' = A x + B u for oracle.mppi.MPPIOracle."""

    def __init__(self, system, A, B):
        self.system, self.A, self.B = system, np.asarray(A), np.asarray(B)
        self.state_dim = self.A.shape[0]

    def pred_batch(self, s, u):
        return s @ self.A.T + u @ self.B.T


@functools.lru_cache(maxsize=None)
def cpu_rollouts(name):
    """Every problem's costs [N], clipped noise [H][N][nu] and updated sequence [H][nu] from the oracle's MPPI on the
    problem's (A, B), fed the plan's warm start and noise."""
    from oracle.costs import QuadCostOracle
    from oracle.mppi import MPPIOracle
    system, ab = matrices(name)
    d = plan_data(name)
    nu = system.ctrl_dim
    out = []
    for b in range(len(N_LIST)):
        A, B = ab[int(d["index"][b])]
        np.random.seed(0)
        orc = MPPIOracle(LinearOracle(system, A, B), QuadCostOracle(d["Q"][b], d["R"][b], d["F"][b], d["goal"][b]),
                         np.tile([LO, HI], (nu, 1)), horizon=int(d["H"][b]), num_path=int(d["N"][b]), sigma=SIGMA,
                         lmda=LMDA)
        orc.act_sequence = np.array(d["act"][b])
        costs, eps = orc.do_rollouts(np.array(d["x0"][b]), np.array(d["eps"][b]))
        orc.update(costs, eps)
        out.append((costs, eps, orc.act_sequence.copy()))
    return out
