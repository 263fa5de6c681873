#!/usr/bin/env python3
"""Golden vectors of the model-accuracy layer, from the REAL reference (williamedwards/autompc).

Run in the build container only (needs the reference checkout that gen_golden.py installs):

    python tests/golden/gen_golden_kstep.py

Writes ``tests/golden/kstep_*.npz`` (data only): the reference's ``get_model_rmse`` / ``get_model_rmsmens``
(evaluation/model_metrics.py) of seeded MLP nets, of ARX / Koopman models it trained, and of a pure-numpy linear
test double, over ragged trajectories at horizons 1..10 and 20; and one ``HoldoutModelEvaluator`` run
(evaluation/holdout_evaluator.py) with the reference's MLP.  MLP weights are not stored: they come from
``oracle.mlp.random_params(seed)`` + ``normalisers(seed)`` on both sides, as in gen_golden.py.  The reference's
RMSMENS calls ``model.pred_parallel``, which its models lack: the instance gets ``pred_parallel = pred_batch``.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G                                        # noqa: E402  (installs the reference)
from autompc.evaluation.holdout_evaluator import HoldoutModelEvaluator   # noqa: E402
from autompc.evaluation.model_metrics import get_model_rmse, get_model_rmsmens   # noqa: E402

HORIZONS = list(range(1, 11)) + [20]
LENS = [31, 12, 26, 7, 19, 40]          # ragged; 7 and 12 are shorter than the largest horizon
# (the reference's ARX builds its lagged features wrongly for a prefix shorter than its history, arx.py:62-68:
#  every truncated trajectory of the linear cases keeps at least 4 rows)
LIN_LENS = [31, 25, 38, 26, 29, 40]

# tag, nx, nu, hidden, activation, seed: every activation, depths 1-4, widths 16 / 37 / 200 / 256
MLP_CASES = [
    ("c4_relu1", 4, 1, [16], "relu", 41),
    ("c4_tanh2", 4, 1, [37, 200], "tanh", 42),
    ("c4_sigmoid3", 4, 1, [256, 16, 37], "sigmoid", 43),
    ("hc_selu4", 17, 6, [37, 16, 200, 256], "selu", 44),
    ("hc_relu2", 17, 6, [256, 256], "relu", 45),
    ("hc_tanh1", 17, 6, [200], "tanh", 46),
    ("w64_sigmoid2", 64, 2, [37, 16], "sigmoid", 47),
]


def ragged_trajs(system, seed, lens=LENS, scale=0.1):
    rng = np.random.default_rng(seed)
    nx, nu = system.obs_dim, system.ctrl_dim
    out = []
    for L in lens:
        t = G.ampc.zeros(system, L)
        t.obs[:] = scale * rng.normal(size=(L, nx)).cumsum(axis=0)
        t.ctrls[:] = rng.normal(size=(L, nu))
        out.append(t)
    return out


def metrics(model, trajs, rmsmens=True):
    rmse = np.array([G.quiet(get_model_rmse, model, trajs, horizon=h) for h in HORIZONS])
    if not rmsmens:
        return rmse, None
    model.pred_parallel = model.pred_batch
    return rmse, np.array([G.quiet(get_model_rmsmens, model, trajs, horiz=h) for h in HORIZONS])


def stack(trajs):
    return (np.array([len(t) for t in trajs]), np.concatenate([t.obs for t in trajs]),
            np.concatenate([t.ctrls for t in trajs]))


def gen_mlp():
    for tag, nx, nu, hidden, act, seed in MLP_CASES:
        system = G.make_system(nx, nu)
        model, p = G.ref_mlp(system, hidden, act, seed)
        trajs = ragged_trajs(system, seed + 500, scale=0.05)
        rmse, rmsmens = metrics(model, trajs)
        lens, obs, ctrls = stack(trajs)
        G.save("kstep_mlp_" + tag, nx=nx, nu=nu, hidden=np.array(hidden), activation=act, seed=seed,
               checksum=G.weight_checksum(p), horizons=np.array(HORIZONS), lens=lens, obs=obs, ctrls=ctrls,
               rmse=rmse, rmsmens=rmsmens)


def gen_linear():
    """ARX (history 2 and 4) and a poly-basis Koopman trained by the reference (the traj_to_states path), one ARX
    wider than 64 states (the host fallback), and a pure-numpy linear double through the reference's metrics."""
    from autompc.sysid.arx import ARX
    from autompc.sysid.koopman import Koopman
    cases = [("arx2", 4, 1, lambda s: ARX(s, history=2)),
             ("arx4", 4, 1, lambda s: ARX(s, history=4)),
             ("koop_poly", 4, 1, lambda s: Koopman(s, method="lstsq", poly_basis="true", poly_degree=2,
                                                         trig_basis="false", product_terms="false")),
             ("arx4_wide", 17, 6, lambda s: ARX(s, history=4))]
    for tag, nx, nu, make in cases:
        system = G.make_system(nx, nu)
        train = G.linear_train_trajs(system, n_traj=6, T=40, seed=321)
        model = G.quiet(make, system)
        G.quiet(model.train, train)
        full = G.linear_train_trajs(system, n_traj=len(LIN_LENS), T=max(LIN_LENS), seed=654)
        trajs = [t[:L] for t, L in zip(full, LIN_LENS)]
        rmse, _ = metrics(model, trajs, rmsmens=False)
        lens, obs, ctrls = stack(trajs)
        G.save("kstep_lin_" + tag, nx=nx, nu=nu, A=model.A, B=model.B, state_dim=model.state_dim,
               horizons=np.array(HORIZONS), lens=lens, obs=obs, ctrls=ctrls, rmse=rmse)

    class NumpyLinear:
        """x' = A x + B u on the host: the CPU test double."""
        def __init__(self, A, B):
            self.A, self.B = A, B

        def pred_batch(self, states, ctrls):
            return states @ self.A.T + ctrls @ self.B.T

    system = G.make_system(3, 2)
    rng = np.random.default_rng(77)
    A = np.eye(3) + 0.05 * rng.normal(size=(3, 3))
    B = 0.1 * rng.normal(size=(3, 2))
    trajs = ragged_trajs(system, 78)
    rmse, rmsmens = metrics(NumpyLinear(A, B), trajs)
    lens, obs, ctrls = stack(trajs)
    G.save("kstep_numpy_linear", A=A, B=B, horizons=np.array(HORIZONS), lens=lens, obs=obs, ctrls=ctrls,
           rmse=rmse, rmsmens=rmsmens)


def gen_holdout():
    """HoldoutModelEvaluator(holdout_prop=0.25, default_rng(seed)) with the reference's MLP trained on the
    training split, three configurations.  The data set holds a duplicate of a trajectory the holdout draws, so
    value equality removes it from the training set too."""
    nx, nu, n_iter, n_batch = 4, 1, 3, 64
    system = G.make_system(nx, nu)
    base = ragged_trajs(system, 901, lens=[40, 33, 45, 28, 50, 38, 42], scale=0.05)
    dup = G.ampc.zeros(system, len(base[2]))
    dup.obs[:], dup.ctrls[:] = base[2].obs, base[2].ctrls
    trajs = base + [dup]                         # index 7 equals index 2 (a separate object)
    for seed in range(1000):
        probe = np.random.default_rng(seed).choice(np.arange(len(trajs)), round(0.25 * len(trajs)), replace=False)
        if 2 in probe and 7 not in probe:
            break
    cfgs = [{"nonlintype": "relu", "n_hidden_layers": "2", "hidden_size_1": 32, "hidden_size_2": 48, "lr": 1e-3},
            {"nonlintype": "tanh", "n_hidden_layers": "1", "hidden_size_1": 64, "lr": 3e-3},
            {"nonlintype": "selu", "n_hidden_layers": "3", "hidden_size_1": 20, "hidden_size_2": 40,
             "hidden_size_3": 24, "lr": 1e-2}]

    def factory(cfg, train_trajs):
        kw = dict(cfg)
        kw["n_hidden_layers"] = int(kw["n_hidden_layers"])
        m = G.quiet(G.MLP, system, n_train_iters=n_iter, n_batch=n_batch, seed=100, use_cuda=False, **kw)
        G.quiet(m.train, train_trajs)
        return m

    ev = HoldoutModelEvaluator(system, trajs, "rmse", np.random.default_rng(seed), horizon=3, holdout_prop=0.25)
    holdout_idx = [i for i, t in enumerate(trajs) if any(t is h for h in ev.holdout)]
    scores = np.array([ev(factory, c) for c in cfgs])
    lens, obs, ctrls = stack(trajs)
    import json
    G.save("kstep_holdout", nx=nx, nu=nu, seed=seed, holdout_prop=0.25, horizon=3, n_train_iters=n_iter,
           n_batch=n_batch, lens=lens, obs=obs, ctrls=ctrls, holdout_idx=np.array(holdout_idx),
           n_train=len(ev.training_set), cfgs=json.dumps(cfgs), scores=scores)


if __name__ == "__main__":
    gen_mlp()
    gen_linear()
    gen_holdout()
