"""What test_mppi_table_host.py (no GPU) and test_gpu_mppi_table.py share: the stacks of MPPI candidates on MLP models
of mixed shapes, the noise they are fed and each candidate's oracle closed loop (MPPIOracle + MLPOracle)."""
import functools

import numpy as np

from helpers import make_system
from oracle import mlp as omlp
from oracle.costs import QuadCostOracle
from oracle.mlp import MLPOracle
from oracle.mppi import MPPIOracle

# (hidden widths, activation, num_path, horizon)
EDGES = [([16], "relu", 16, 2), ([17, 33], "tanh", 17, 5), ([256, 256], "relu", 40, 30), ([1, 40], "sigmoid", 5, 7),
         ([64, 16, 48, 128], "selu", 33, 16), ([255], "sigmoid", 64, 29)]
# two more systems, widths of test_gpu_kstep_mlp.py's sweep: 16 / 16 (in = 32: two full blocks, one output tile) and
# 48 / 16 (in = 64: four full blocks, three output tiles -- wave 3 has none --, 64 of the 80 xu columns)
EDGES_16 = [([15], "tanh", 5, 2), ([65, 129], "relu", 16, 7), ([193], "sigmoid", 17, 4), ([129, 15, 65], "selu", 33, 5)]
EDGES_48 = [([193, 65], "selu", 33, 3), ([15], "relu", 17, 7), ([65, 193, 129], "tanh", 16, 2), ([129], "sigmoid", 5, 6)]
T = 4


def hip_model(system, p, precision="f64"):
    from autompc_amd import MLP
    m = MLP(system, n_hidden_layers=len(p["weights"]) - 1, nonlintype=p["activation"], precision=precision,
            **{"hidden_size_%d" % (i + 1): w.shape[0] for i, w in enumerate(p["weights"][:-1])})
    m.weights, m.biases = [w.copy() for w in p["weights"]], [b.copy() for b in p["biases"]]
    m.xu_means, m.xu_std, m.dy_means, m.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
    m.jit_kernels = False              # (as the models a tuner fits for one evaluation: no run-time kernel builds)
    return m


def make_task(system, cost=None):
    from autompc_amd import QuadCost, Task
    nx, nu = system.obs_dim, system.ctrl_dim
    task = Task(system)
    task.set_cost(cost if cost is not None else QuadCost(system, np.eye(nx), 0.01 * np.eye(nu), 2.0 * np.eye(nx)))
    task.set_ctrl_bounds(-np.ones(nu), np.ones(nu))
    return task


def stack(nx, nu, edges, seed):
    from autompc_amd.tuning import random_candidates
    system = make_system(nx, nu)
    params = [omlp.random_params(nx, nu, h, a, seed=seed + i) for i, (h, a, _, _) in enumerate(edges)]
    p_sur = omlp.random_params(nx, nu, [128, 64], "tanh", seed=seed + 90)
    cands = random_candidates(system, len(edges), seed=3)
    for c, p, (_, _, n, hz) in zip(cands, params, edges):
        c["num_path"], c["horizon"] = n, hz
        c["Q"], c["R"], c["F"] = c["Q"] ** 0.1, c["R"] ** 0.1, c["F"] ** 0.1           # costs stay O(1)
        c["model"] = hip_model(system, p)
    init = np.random.default_rng(0).uniform(-0.1, 0.1, size=nx)
    return dict(system=system, params=params, p_sur=p_sur, cands=cands, init=init, task=make_task(system),
                own=hip_model(system, params[0]), sur=hip_model(system, p_sur))


@functools.lru_cache(maxsize=None)
def six():
    return stack(17, 6, EDGES, seed=40)


@functools.lru_cache(maxsize=None)
def sixteen():
    return stack(16, 16, EDGES_16, seed=110)


@functools.lru_cache(maxsize=None)
def forty_eight():
    return stack(48, 16, EDGES_48, seed=130)


def fed_noise(cands, nu, steps, seed=9):
    rng = np.random.default_rng(seed)
    acts = [rng.normal(scale=np.sqrt(c["sigma"]), size=(c["horizon"], nu)) for c in cands]
    eps = [[rng.normal(scale=np.sqrt(c["sigma"]), size=(c["num_path"], c["horizon"], nu)) for c in cands]
           for _ in range(steps)]
    return acts, eps


def oracle_loop(S, b, steps, acts, eps, p=None):
    """Candidate b's closed loop on its own MPPIOracle + MLPOracle (parameters `p`: a restatement of the candidate's
    network), fed the noise of fed_noise: (obs [steps + 1][nx], ctrls [steps + 1][nu], the task cost's score)."""
    system, c, init = S["system"], S["cands"][b], S["init"]
    nx, nu = system.obs_dim, system.ctrl_dim
    sur = MLPOracle(system, S["p_sur"])
    task_cost = QuadCostOracle(np.eye(nx), 0.01 * np.eye(nu), 2.0 * np.eye(nx), np.zeros(nx))
    np.random.seed(0)
    orc = MPPIOracle(MLPOracle(system, S["params"][b] if p is None else p),
                     QuadCostOracle(np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), np.zeros(nx)),
                     np.tile([-1.0, 1.0], (nu, 1)), horizon=c["horizon"], num_path=c["num_path"],
                     sigma=c["sigma"], lmda=c["lmda"])
    orc.act_sequence = acts[b].copy()
    x, cs = init.copy(), np.concatenate([init, np.zeros(nu)])
    o_obs, o_ctl = [x.copy()], []
    for s in range(steps):
        u, cs = orc.run(cs, x, eps_nhu=eps[s][b])
        x = sur.pred(x, u)
        o_ctl.append(u)
        o_obs.append(x.copy())
    o_ctl.append(np.zeros(nu))
    o_obs, o_ctl = np.array(o_obs), np.array(o_ctl)
    return o_obs, o_ctl, task_cost.traj_cost(o_obs, o_ctl)
