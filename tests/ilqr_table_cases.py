"""The candidates that test_ilqr_table_host.py (no GPU) and test_gpu_ilqr_table.py share: six MLP models on the edges
of the table kernels at 17 states / 6 controls, their iLQR candidates and each candidate's oracle closed loop (ILQROracle
+ MLPOracle, computed once per process and never modified)."""
import functools

import numpy as np

from helpers import make_system
from oracle import mlp as omlp
from oracle.costs import QuadCostOracle
from oracle.ilqr import ILQROracle
from oracle.mlp import MLPOracle

# (hidden widths, activation, horizon)
EDGES = [([16], "relu", 2), ([17, 33], "tanh", 5), ([256, 256], "relu", 25), ([1, 40], "sigmoid", 7),
         ([64, 16, 48, 128], "selu", 16), ([255], "sigmoid", 24)]
WIDE = [([17, 33], "tanh", 3), ([255], "sigmoid", 17)]        # the second system, 33 / 5
MAX_ITER, STEPS = 8, 3


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
    from autompc_amd.tuning.batch_eval import random_ilqr_candidates
    system = make_system(nx, nu)
    params = [omlp.random_params(nx, nu, h, a, seed=seed + i) for i, (h, a, _) in enumerate(edges)]
    p_sur = omlp.random_params(nx, nu, [128, 64], "tanh", seed=seed + 90)
    cands = random_ilqr_candidates(system, len(edges), seed=3)
    for c, p, (_, _, hz) in zip(cands, params, edges):
        c["horizon"] = hz
        c["Q"], c["R"], c["F"] = c["Q"] ** 0.1, c["R"] ** 0.1, c["F"] ** 0.1           # costs stay O(1)
        c["model"] = hip_model(system, p)
    init = np.random.default_rng(0).uniform(-0.1, 0.1, size=nx)
    return dict(system=system, params=params, p_sur=p_sur, cands=cands, init=init, task=make_task(system),
                own=hip_model(system, params[0]), sur=hip_model(system, p_sur))


@functools.lru_cache(maxsize=None)
def six():
    return stack(17, 6, EDGES, seed=40)


@functools.lru_cache(maxsize=None)
def wide():
    return stack(33, 5, WIDE, seed=60)


def permuted(p, seed=5):
    """The same network with every hidden layer's units in another order: every summation order changes."""
    rng = np.random.default_rng(seed)
    W, B = [w.copy() for w in p["weights"]], [b.copy() for b in p["biases"]]
    for l in range(len(W) - 1):
        perm = rng.permutation(W[l].shape[0])
        W[l], B[l] = W[l][perm], B[l][perm]
        W[l + 1] = W[l + 1][:, perm]
    return dict(p, weights=W, biases=B)


def oracle_of(S, b, p=None, **kw):
    c, nx, nu = S["cands"][b], S["system"].obs_dim, S["system"].ctrl_dim
    kw.setdefault("max_iter", MAX_ITER)
    return ILQROracle(MLPOracle(S["system"], S["params"][b] if p is None else p),
                      QuadCostOracle(np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), np.zeros(nx)),
                      S["system"].dt, c["horizon"], ubounds=(-np.ones(nu), np.ones(nu)), **kw)


def oracle_loop(S, b, p=None, steps=STEPS):
    """Candidate b's closed loop as IterativeLQR.run + simulate() make it: a full solve from a zero guess per control
    step, x <- surrogate.pred(x, u).  Returns per-step solves, the rows and the task cost's score."""
    system, nu = S["system"], S["system"].ctrl_dim
    nx = system.obs_dim
    orc, sur = oracle_of(S, b, p), MLPOracle(system, S["p_sur"])
    x = S["init"].copy()
    obs, ctl, solves = [x.copy()], [], []
    for _ in range(steps):
        conv, st, ct, Ks, ks = orc.solve(x, np.zeros((orc.H, nu)))
        solves.append(dict(converged=bool(conv), iters=int(orc.n_iter), obj=float(orc.final_obj), states=st, ctrls=ct,
                           Ks=Ks, ks=ks, decisions=[t[2:] for t in orc.trace]))
        u = ct[0]
        x = sur.pred(x, u)
        ctl.append(u.copy())
        obs.append(x.copy())
    ctl.append(np.zeros(nu))
    task_cost = QuadCostOracle(np.eye(nx), 0.01 * np.eye(nu), 2.0 * np.eye(nx), np.zeros(nx))
    return dict(solves=solves, obs=np.array(obs), ctrls=np.array(ctl),
                score=float(task_cost.traj_cost(np.array(obs), np.array(ctl))))


@functools.lru_cache(maxsize=None)
def six_loops():
    return [oracle_loop(six(), b) for b in range(len(EDGES))]
