"""Shared by the wide-linear k-step tests: the goldens of tests/golden/gen_golden_kstep_wide.py as models."""
import os

import numpy as np

from autompc_amd import ARX, Koopman, System, Trajectory
from autompc_amd.sysid.linear import _LinearModel

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# tag -> how the model is rebuilt around the stored A, B (the reference trained them)
WIDE = {
    "arx4_hc": lambda s, p: ARX(s, history=4, precision=p),
    "arx7_hc": lambda s, p: ARX(s, history=7, precision=p),
    "arx10_hc": lambda s, p: ARX(s, history=10, precision=p),
    "arx10_nu1": lambda s, p: ARX(s, history=10, precision=p),
    "koop_trig": lambda s, p: Koopman(s, method="lstsq", trig_basis=True, poly_degree=1, precision=p),
    "koop_polytrig": lambda s, p: Koopman(s, method="lstsq", poly_basis=True, poly_degree=2, trig_basis=True,
                                          precision=p),
    "koop_id70": lambda s, p: ObsLinear(s, precision=p),
}
RULES = {"arx4_hc": 1, "arx7_hc": 1, "arx10_hc": 1, "arx10_nu1": 1, "koop_trig": 2, "koop_polytrig": 2, "koop_id70": 0}


class ObsLinear(_LinearModel):
    """x' = A x + B u on the observation itself: a linear model without traj_to_states (the reference's Koopman
    with the identity basis only)."""

    @property
    def state_dim(self):
        return self.system.obs_dim

    def traj_to_state(self, traj):
        return np.asarray(traj.obs[-1], dtype=np.float64).copy()

    def update_state(self, state, new_ctrl, new_obs):
        return np.asarray(new_obs, dtype=np.float64).copy()

    def train(self, trajs, silent=False):
        raise NotImplementedError("the tests set A and B")


class RowsARX(ARX):
    """An ARX whose traj_to_states is its own method: scored from uploaded rows (rule 0), same values."""

    def traj_to_states(self, traj):
        return ARX.traj_to_states(self, traj)


def system(no, nu):
    return System(["x%d" % i for i in range(no)], ["u%d" % i for i in range(nu)], dt=0.05)


def gold(tag):
    return np.load(os.path.join(GOLD, "kstep_wide_%s.npz" % tag))


def trajs_of(s, g):
    out, r = [], 0
    for n in g["lens"]:
        n = int(n)
        out.append(Trajectory(s, n, g["obs"][r:r + n].copy(), g["ctrls"][r:r + n].copy()))
        r += n
    return out


def wide_model(tag, precision="f64", make=None):
    """(model carrying the golden's A and B, its test trajectories, the golden)."""
    g = gold(tag)
    s = system(int(g["nx"]), int(g["nu"]))
    m = (make or WIDE[tag])(s, precision)
    m.A, m.B = g["A"].copy(), g["B"].copy()
    assert m.A.shape[0] == int(g["state_dim"])
    return m, trajs_of(s, g), g


def ragged_trajs(s, lengths, seed):
    """Seeded data of any shape (a damped nonlinear oscillator driven by random controls)."""
    no, nu = s.obs_dim, s.ctrl_dim
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(no, no))
    M = np.eye(no) + 0.1 * (-0.4 * np.eye(no) + 0.5 * (S - S.T) / np.sqrt(no / 3.0))
    G = rng.normal(scale=0.3, size=(no, nu))
    out = []
    for L in lengths:
        obs, ctl = np.zeros((L, no)), rng.uniform(-1.0, 1.0, size=(L, nu))
        x = rng.uniform(-1.0, 1.0, size=no)
        for i in range(L):
            obs[i] = x
            x = M @ x + 0.4 * np.sin(2.0 * x[::-1]) + G @ ctl[i]
        out.append(Trajectory(s, L, obs, ctl))
    return out
