#!/usr/bin/env python3
"""Golden vectors of the linear model fits, from the REAL reference (williamedwards/autompc).

Run in the build container only (needs the reference checkout that gen_golden.py installs):

    python tests/golden/gen_golden_linfit.py

Writes ``tests/golden/linfit_*.npz`` (data only): the training data (``traj_len``, concatenated ``obs`` / ``ctrls``)
and what the reference's ``ARX.train`` / ``Koopman.train`` make of it -- per ARX history ``coeffs_<k>`` (the first
obs_dim rows of [A | B], arx.py:137-143), per Koopman case ``A_<tag>`` / ``B_<tag>``.  The data come from a damped,
nonlinear oscillator driven by random controls (gen_golden.linear_train_trajs' dynamics with a stronger nonlinear
term and a rotation scaled to stay stable at 17 states), so the reference's least-squares problems have full column
rank and lagged observations are not linear in one another to rounding.

Cases: a 3-observation / 1-control system with ragged lengths that include 1, 2 and 3 (histories 1, 2, 5, 10: longer
than some trajectories); the 17 / 6 shape on 12 trajectories x 80 steps (histories 1, 4, 10); on both, the strict
Koopman configurations without duplicate basis functions: identity, poly_degree = 2, trig with poly_degree = 1.

Per case the script prints the error of ``gram_fit_host`` against the reference, max|dcoef| / max|coef|, and the
smallest squared pivot, asserts that the acceptance rule takes the case, and stores the error as ``host_err_<tag>``:
the GPU tests allow the device 100 x that, with a floor of 1e-13.  Printed when the goldens were made:

    small  arx1       1.6e-15  pivot 8.0e-01      hc     arx1       1.6e-15  pivot 5.5e-01
    small  arx2       5.7e-14  pivot 3.2e-03      hc     arx4       3.6e-13  pivot 1.1e-02
    small  arx5       1.6e-12  pivot 2.0e-03      hc     arx10      1.1e-12  pivot 8.8e-03
    small  arx10      3.2e-12  pivot 2.0e-03      hc     koop_id    2.6e-15  pivot 5.5e-01
    small  koop_id    8.7e-16  pivot 8.0e-01      hc     koop_poly2 3.6e-15  pivot 4.9e-01
    small  koop_poly2 2.8e-15  pivot 4.6e-01      hc     koop_trig1 2.9e-15  pivot 5.2e-01
    small  koop_trig1 6.5e-13  pivot 2.3e-03
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G                                        # noqa: E402  (installs the reference)
from autompc.sysid.arx import ARX                             # noqa: E402
from autompc.sysid.koopman import Koopman                     # noqa: E402

from autompc_amd.sysid import linear_fit as LF                # noqa: E402

KOOPMAN = {      # tag -> (reference constructor arguments, (kinds, params) of the strict basis)
    "id": (dict(poly_basis="false", trig_basis="false"), ([0], [1.0])),
    "poly2": (dict(poly_basis="true", poly_degree=2, trig_basis="false"), ([0, 1], [1.0, 2.0])),
    "trig1": (dict(poly_basis="false", poly_degree=1, trig_basis="true", trig_freq=1), ([0, 2, 3], [1.0, 1.0, 1.0])),
}


NONLIN = 0.4     # gen_golden.linear_train_trajs has 0.05: lagged observations are then linear in one another to ~1e-8


def train_trajs(system, lengths, seed):
    """gen_golden.linear_train_trajs' dynamics with a length per trajectory."""
    no, nu = system.obs_dim, system.ctrl_dim
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(no, no))
    M = np.eye(no) + 0.1 * (-0.4 * np.eye(no) + 0.5 * (S - S.T) / np.sqrt(no / 3.0))     # stable at 17 states too
    Gm = rng.normal(scale=0.3, size=(no, nu))
    trajs = []
    for T in lengths:
        traj = G.ampc.zeros(system, T)
        x = rng.uniform(-1.0, 1.0, size=no)
        for t in range(T):
            u = rng.uniform(-1.0, 1.0, size=nu)
            traj[t].obs[:] = x
            traj[t].ctrl[:] = u
            x = M @ x + NONLIN * np.sin(2.0 * x[::-1]) + Gm @ u
        trajs.append(traj)
    return trajs


def ref_arx_coeffs(system, k, trajs):
    """The reference's regression coefficients [obs_dim][fvec].  ARX.train raises for history 1 with more than one
    control (arx.py:141 writes the lag-1 control slot of B, which a history-1 state does not have) AFTER its
    regression (arx.py:111-116); there the same regression is run on the reference's own training matrix."""
    no = system.obs_dim
    m = ARX(system, history=k)
    try:
        G.quiet(m.train, trajs)
    except ValueError:
        assert k == 1
        matrix, targets = m._get_training_matrix_and_targets(trajs)
        return np.stack([np.linalg.lstsq(matrix, targets[:, i], rcond=None)[0] for i in range(no)])
    return np.hstack([m.A[:no], m.B[:no]])


def rel_err(a, ref):
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


def gen_case(name, no, nu, lengths, histories, seed):
    system = G.make_system(no, nu)
    trajs = train_trajs(system, lengths, seed)
    lens = np.array([len(t) for t in trajs], dtype=np.int32)
    obs = np.concatenate([np.asarray(t.obs) for t in trajs])
    ctrls = np.concatenate([np.asarray(t.ctrls) for t in trajs])
    out = dict(traj_len=lens, obs=obs, ctrls=ctrls, histories=np.array(histories))
    bases = [KOOPMAN[tag][1] for tag in KOOPMAN]
    coeffs, status, pivot = LF.gram_fit_host(lens, obs, ctrls, histories, bases)
    for i, k in enumerate(histories):
        ref = ref_arx_coeffs(system, k, trajs)
        err = rel_err(coeffs[i], ref)
        print("%-6s arx%-7d %.1e  pivot %.1e" % (name, k, err, pivot[i]))
        assert status[i] == 0, "golden case not accepted by the rule"
        out["coeffs_%d" % k], out["host_err_arx%d" % k] = ref, err
    for j, tag in enumerate(KOOPMAN):
        m = G.quiet(Koopman, system, method="lstsq", product_terms="false", **KOOPMAN[tag][0])
        G.quiet(m.train, trajs)
        ref = np.hstack([m.A, m.B])
        i = len(histories) + j
        err = rel_err(coeffs[i], ref)
        print("%-6s koop_%-5s %.1e  pivot %.1e" % (name, tag, err, pivot[i]))
        assert status[i] == 0, "golden case not accepted by the rule"
        out["A_" + tag], out["B_" + tag], out["host_err_koop_" + tag] = np.asarray(m.A), np.asarray(m.B), err
    G.save("linfit_" + name, **out)


def gen():
    gen_case("small", 3, 1, [40, 1, 25, 2, 3, 31, 2, 12, 50, 1, 36, 44], [1, 2, 5, 10], 201)
    gen_case("hc", 17, 6, [80] * 12, [1, 4, 10], 202)


if __name__ == "__main__":
    gen()
