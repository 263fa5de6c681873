"""Shared by the SINDy k-step tests: the goldens of tests/golden/gen_golden_kstep_sindy.py as models."""
import os

import numpy as np

from autompc_amd import SINDy, System, Trajectory

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# tag -> (n_tab > 0: product table / 0: direct evaluation, program staged in LDS) for f64 handles
CASES = {
    "c1_trig": (True, True),
    "poly3_trig2_cont": (True, True),
    "cross3": (True, True),
    "cross5": (False, False),
    "hc_trig": (True, True),
    "hc_trigx": (True, False),
}


def system(no, nu, dt=0.05):
    return System(["x%d" % i for i in range(no)], ["u%d" % i for i in range(nu)], dt=dt)


def gold(tag):
    return np.load(os.path.join(GOLD, "kstep_sindy_%s.npz" % tag))


def hyper_of(g):
    """The golden's hyper-parameters as SINDy constructor arguments."""
    return dict(trig_basis=int(g["trig_freq"]) > 0, trig_freq=max(int(g["trig_freq"]), 1),
                trig_interaction=bool(g["trig_interaction"]), poly_basis=int(g["poly_degree"]) > 1,
                poly_degree=int(g["poly_degree"]), poly_cross_terms=bool(g["poly_cross_terms"]),
                time_mode=str(g["time_mode"]))


def trajs_of(s, g):
    out, r = [], 0
    for n in g["lens"]:
        n = int(n)
        out.append(Trajectory(s, n, g["obs"][r:r + n].copy(), g["ctrls"][r:r + n].copy()))
        r += n
    return out


def sindy_model(tag, precision="f64"):
    """(SINDy carrying the golden's coefficients, its test trajectories, the golden)."""
    g = gold(tag)
    s = system(int(g["nx"]), int(g["nu"]), float(g["dt"]))
    m = SINDy(s, precision=precision, **hyper_of(g))
    m.set_coefficients(g["Xi"])
    return m, trajs_of(s, g), g
