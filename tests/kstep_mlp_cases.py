"""Shared builders of the ``ampc_kstep_errors_mlp`` tests: the models and trajectories of the reference-generated
fixtures tests/golden/kstep_mlp_*.npz (the recipe of test_gpu_model_metrics.py), and a seeded synthetic data set."""
import numpy as np

from conftest import golden
from helpers import golden_params, make_system, weight_checksum

TAGS = ["c4_relu1", "c4_sigmoid3", "c4_tanh2", "hc_relu2", "hc_selu4", "hc_tanh1", "w64_sigmoid2"]


def trajs_of(system, g):
    from autompc_amd import Trajectory
    out, o = [], 0
    for L in g["lens"]:
        L = int(L)
        out.append(Trajectory(system, L, g["obs"][o:o + L].copy(), g["ctrls"][o:o + L].copy()))
        o += L
    return out


def mlp_of(system, p, hidden, act, precision="f64"):
    from autompc_amd import MLP
    m = MLP(system, n_hidden_layers=len(hidden), nonlintype=str(act), precision=precision,
            **{"hidden_size_%d" % (i + 1): int(h) for i, h in enumerate(hidden)})
    m.jit_kernels = False
    m.weights, m.biases = [w.copy() for w in p["weights"]], [b.copy() for b in p["biases"]]
    m.xu_means, m.xu_std, m.dy_means, m.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
    return m


def fixture_model(tag, precision="f64", seed=None):
    """(model, trajectories, golden) of fixture `tag`; `seed`: another model of the fixture's shape."""
    g = golden("kstep_mlp_" + tag)
    nx, nu = int(g["nx"]), int(g["nu"])
    system = make_system(nx, nu)
    p = golden_params(nx, nu, g["hidden"], str(g["activation"]), int(g["seed"]) if seed is None else seed)
    if seed is None:
        np.testing.assert_allclose(weight_checksum(p), g["checksum"], rtol=0, atol=1e-12)
    return mlp_of(system, p, g["hidden"], g["activation"], precision), trajs_of(system, g), g


def synthetic_trajs(system, lens=(40, 23, 31, 17), seed=0):
    """Random-walk observations and uniform controls (the data test_gpu_mlp_fit.py fits)."""
    from autompc_amd import Trajectory
    rng = np.random.default_rng(seed)
    out = []
    for L in lens:
        obs = 0.05 * rng.normal(size=(L, system.obs_dim)).cumsum(axis=0)
        ctrls = rng.uniform(-1, 1, size=(L, system.ctrl_dim))
        out.append(Trajectory(system, L, obs, ctrls))
    return out
