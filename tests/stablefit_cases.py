"""Shared by the stable-fit tests: the cases of tests/golden/gen_golden_stablefit.py (the reference's own
stabilize_discrete on each) and the models that go with them."""
import os

import numpy as np

from autompc_amd import Koopman, Trajectory

from linfit_cases import system

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# name -> observations, controls, trajectory lengths, data seed, spectral radius of the linear part of the dynamics,
# start amplitude, Koopman arguments (gain: the scale of the control matrix, 0.1 when absent).  Smallest first.
CASES = {
    # the smallest: identity basis, 33 design rows, one partial tile everywhere
    "n2": dict(no=2, nu=1, lengths=[12] * 3, seed=401, rho=1.06, amp=0.5, koopman=dict()),
    # x, x^2, sin x, cos x of 3 observations: n = 12, no multiple of 16
    "n12": dict(no=3, nu=1, lengths=[40] * 6, seed=402, rho=1.015, amp=0.4,
                koopman=dict(strict_reference=False, poly_basis=True, poly_degree=2, trig_basis=True, trig_freq=1)),
    # 17 observations x 3 basis functions, 6 controls, 1980 design rows: several row splits of the Gram pass
    "n51": dict(no=17, nu=6, lengths=[100] * 20, seed=403, rho=1.004, amp=0.5,
                koopman=dict(strict_reference=False, trig_basis=True, trig_freq=1)),
    # the size limit: 4 observations x 16 basis functions (x, x^2, sin / cos of x .. 7 x)
    "n64": dict(no=4, nu=2, lengths=[12] * 60, seed=404, rho=1.01, amp=2.0, gain=0.05,
                koopman=dict(strict_reference=False, poly_basis=True, poly_degree=2, trig_basis=True, trig_freq=7)),
    # the least-squares A is already stable: the clip at 1 stays idle
    "inactive": dict(no=3, nu=1, lengths=[40] * 4, seed=415, rho=0.9, amp=1.0,
                     koopman=dict(strict_reference=False, poly_basis=True, poly_degree=2)),
    # the strict-reference basis of poly_degree 3: x, x^3 twice -> a singular Gram -> status 1 -> the host route.  (The
    # reference's own result on a singular design hangs on its pseudo-inverse cutoff and its unsymmetric ``eig``: it is
    # recorded, and compared with nothing.)
    "dup": dict(no=2, nu=1, lengths=[30] * 5, seed=406, rho=1.01, amp=0.4,
                koopman=dict(poly_basis=True, poly_degree=3)),
}
FITTED = [n for n in CASES if n != "dup"]


def make_data(name):
    """(traj_len, obs, ctrls) of a case (its name, or a dict like a case's): a slightly unstable rotation plus a small
    sine term, random controls and measurement noise; short trajectories keep it bounded."""
    c = CASES[name] if isinstance(name, str) else name
    no, nu = c["no"], c["nu"]
    rng = np.random.default_rng(c["seed"])
    K = rng.normal(size=(no, no))
    w, V = np.linalg.eig(0.3 * (K - K.T) / np.sqrt(no))         # a rotation generator
    M = c["rho"] * np.real((V * np.exp(w)) @ np.linalg.inv(V))
    Gm = rng.normal(scale=c.get("gain", 0.1), size=(no, nu))
    obs, ctrls = [], []
    for T in c["lengths"]:
        x = rng.uniform(-c["amp"], c["amp"], size=no)
        for _ in range(T):
            u = rng.uniform(-1.0, 1.0, size=nu)
            obs.append(x + rng.normal(scale=0.01, size=no))
            ctrls.append(u)
            x = M @ x + 0.05 * np.sin(2.0 * x[::-1]) + Gm @ u
    return np.array(c["lengths"], dtype=np.int32), np.array(obs), np.array(ctrls)


def gold(name):
    return np.load(os.path.join(GOLD, "stablefit_%s.npz" % name))


def data(name):
    g = gold(name)
    return g["traj_len"], g["obs"], g["ctrls"]


def trajs(name):
    c = CASES[name]
    s = system(c["no"], c["nu"])
    lens, obs, ctrls = data(name)
    out, r = [], 0
    for n in lens:
        out.append(Trajectory(s, int(n), obs[r:r + n].copy(), ctrls[r:r + n].copy()))
        r += int(n)
    return s, out


def new_model(s, name, method="stable"):
    return Koopman(s, method=method, **CASES[name]["koopman"])


def basis(name):
    return new_model(system(CASES[name]["no"], CASES[name]["nu"]), name).device_lift()


def reference(name):
    """[A | B] of the reference."""
    g = gold(name)
    return np.hstack([g["A"], g["B"]])


def tolerance(name):
    """What the Gram form (host or device) may differ from the reference by: 100 x the larger of the restatement's
    recorded error and the case's recorded round-off response."""
    g = gold(name)
    return 100.0 * max(float(g["host_err"]), float(g["roundoff_response"]))


def rel_err(a, ref):
    return float(np.max(np.abs(np.asarray(a) - ref)) / max(np.max(np.abs(ref)), 1e-300))
