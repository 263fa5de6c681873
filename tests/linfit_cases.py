"""Shared by the linear-fit tests: the goldens of tests/golden/gen_golden_linfit.py and seeded training data."""
import os

import numpy as np

from autompc_amd import ARX, Koopman, System, Trajectory

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# tag -> (Koopman arguments (strict_reference default), (kinds, params) of the basis)
KOOPMAN = {
    "id": (dict(), ([0], [1.0])),
    "poly2": (dict(poly_basis=True, poly_degree=2), ([0, 1], [1.0, 2.0])),
    "trig1": (dict(trig_basis=True, poly_degree=1), ([0, 2, 3], [1.0, 1.0, 1.0])),
}
SHAPES = {"small": (3, 1), "hc": (17, 6)}
# (golden file, case tag): every reference case
CASES = ([("small", "arx%d" % k) for k in (1, 2, 5, 10)] + [("hc", "arx%d" % k) for k in (1, 4, 10)]
         + [(n, "koop_" + t) for n in ("small", "hc") for t in KOOPMAN])


def system(no, nu):
    return System(["x%d" % i for i in range(no)], ["u%d" % i for i in range(nu)], dt=0.05)


def gold(name):
    return np.load(os.path.join(GOLD, "linfit_%s.npz" % name))


def gold_trajs(name):
    g = gold(name)
    s = system(*SHAPES[name])
    out, r = [], 0
    for n in g["traj_len"]:
        out.append(Trajectory(s, int(n), g["obs"][r:r + n].copy(), g["ctrls"][r:r + n].copy()))
        r += int(n)
    return s, out


def reference_coeffs(g, tag):
    """The reference's coefficient matrix of a case: ARX [no][fvec], Koopman [A | B]."""
    if tag.startswith("arx"):
        return g["coeffs_" + tag[3:]]
    return np.hstack([g["A_" + tag[5:]], g["B_" + tag[5:]]])


def tolerance(g, tag):
    """100 x the error gen_golden_linfit.py recorded for gram_fit_host against the reference, floor 1e-13."""
    return max(100.0 * float(g["host_err_" + tag]), 1e-13)


def split_request(tags):
    """(ARX histories, Koopman bases) of case tags, in the order ampc_linfit_fit returns them."""
    return ([int(t[3:]) for t in tags if t.startswith("arx")],
            [KOOPMAN[t[5:]][1] for t in tags if t.startswith("koop_")])


def rel_err(a, ref):
    return float(np.max(np.abs(np.asarray(a) - ref)) / np.max(np.abs(ref)))


def make_trajs(s, lengths, seed, nonlin=0.4):
    """A damped nonlinear oscillator driven by random controls (the goldens' dynamics)."""
    no, nu = s.obs_dim, s.ctrl_dim
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(no, no))
    M = np.eye(no) + 0.1 * (-0.4 * np.eye(no) + 0.5 * (S - S.T) / np.sqrt(no / 3.0))
    Gm = rng.normal(scale=0.3, size=(no, nu))
    out = []
    for T in lengths:
        obs, ctrls = np.zeros((T, no)), np.zeros((T, nu))
        x = rng.uniform(-1.0, 1.0, size=no)
        for t in range(T):
            u = rng.uniform(-1.0, 1.0, size=nu)
            obs[t], ctrls[t] = x, u
            x = M @ x + nonlin * np.sin(2.0 * x[::-1]) + Gm @ u
        out.append(Trajectory(s, T, obs, ctrls))
    return out


def model_params(m):
    return m.coeffs if isinstance(m, ARX) else np.hstack([m.A, m.B])


def new_model(s, tag):
    return ARX(s, history=int(tag[3:])) if tag.startswith("arx") else Koopman(s, **KOOPMAN[tag[5:]][0])
