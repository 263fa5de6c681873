#!/usr/bin/env python3
"""Golden vectors of the k-step accuracy of WIDE linear models (65..256 states), from the REAL reference
(williamedwards/autompc).

Run in the build container only (needs the reference checkout that gen_golden.py installs):

    python tests/golden/gen_golden_kstep_wide.py

Writes ``tests/golden/kstep_wide_*.npz`` (data only): the reference's ``get_model_rmse`` (and, for the model whose
state is the observation, ``get_model_rmsmens``) of ARX / Koopman models it trained, at horizons 1..10 and 20 over
ragged trajectories, with the trained ``A``, ``B``, like ``kstep_lin_*.npz``.  Training and test data come from
``gen_golden_linfit.train_trajs`` (a damped nonlinear oscillator: lagged columns are independent, the fits have
full rank).

Two properties of the reference restrict the trajectory lengths:
  * ``ARX._get_all_feature_vectors`` raises a broadcast error on a prefix shorter than ``history - 1`` rows
    (arx.py:67).  With ARX_LENS every length L has L - h >= 9 or L <= h for every horizon h used and every history
    up to 10; 19 and 20 still drop out at horizon 20, which exercises the masking.
  * ``Koopman.traj_to_states`` raises on an empty prefix (np.apply_along_axis on zero rows): KOOP_LENS are all above
    the largest horizon.

Per case the script also prints how far the plain numpy composition ``s A' + u B'`` from ``traj_to_states`` is from
the reference's value (relative): the host algorithm's own error, which the device tolerance of 1e-9 is not spent
on.  Printed when the goldens were made: 0 .. 2.2e-16 in every case (RMSE 2.2 .. 5.4 at one step, 10.9 .. 24.1 at
horizon 20; RMSMENS of the 70-state model 1.28 .. 1.43).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G                                        # noqa: E402  (installs the reference)
from autompc.evaluation.model_metrics import get_model_rmse, get_model_rmsmens   # noqa: E402
from autompc.sysid.arx import ARX                             # noqa: E402
from autompc.sysid.koopman import Koopman                     # noqa: E402

from gen_golden_linfit import train_trajs                     # noqa: E402

HORIZONS = list(range(1, 11)) + [20]
ARX_LENS = [31, 19, 38, 20, 29, 45]
KOOP_LENS = [31, 25, 38, 26, 29, 45]
TRAIN_LENS = [80] * 12

# tag, obs_dim, ctrl_dim, constructor, test lengths, rmsmens too
CASES = [
    ("arx4_hc", 17, 6, lambda s: ARX(s, history=4), ARX_LENS, False),
    ("arx7_hc", 17, 6, lambda s: ARX(s, history=7), ARX_LENS, False),
    ("arx10_hc", 17, 6, lambda s: ARX(s, history=10), ARX_LENS, False),
    ("arx10_nu1", 20, 1, lambda s: ARX(s, history=10), ARX_LENS, False),
    ("koop_trig", 30, 2, lambda s: Koopman(s, method="lstsq", poly_basis="false", poly_degree=1, trig_basis="true",
                                           trig_freq=1, product_terms="false"), KOOP_LENS, False),
    ("koop_polytrig", 17, 6, lambda s: Koopman(s, method="lstsq", poly_basis="true", poly_degree=2,
                                               trig_basis="true", trig_freq=1, product_terms="false"),
     KOOP_LENS, False),
    ("koop_id70", 70, 2, lambda s: Koopman(s, method="lstsq", poly_basis="false", trig_basis="false",
                                           product_terms="false"), KOOP_LENS, True),
]


def numpy_rmse(model, A, B, trajs, h, obs_dim):
    """The reference's algorithm with the model step written as s A' + u B'."""
    sq = []
    for t in trajs:
        if len(t) <= h:
            continue
        s = model.traj_to_states(t[:-h])
        for k in range(h):
            s = s @ A.T + t.ctrls[k:-(h - k), :] @ B.T
        sq.append((s[:, :obs_dim] - t.obs[h:]) ** 2)
    return float(np.sqrt(np.mean(np.concatenate(sq), axis=None) * obs_dim))


def gen():
    for i, (tag, no, nu, make, lens, with_rmsmens) in enumerate(CASES):
        system = G.make_system(no, nu)
        model = G.quiet(make, system)
        G.quiet(model.train, train_trajs(system, TRAIN_LENS, 700 + i))
        trajs = train_trajs(system, lens, 800 + i)
        A, B = np.asarray(model.A, dtype=np.float64), np.asarray(model.B, dtype=np.float64)
        rmse = np.array([G.quiet(get_model_rmse, model, trajs, horizon=h) for h in HORIZONS])
        assert np.all(np.isfinite(rmse)), tag
        host = np.array([numpy_rmse(model, A, B, trajs, h, no) for h in HORIZONS])
        out = dict(nx=no, nu=nu, A=A, B=B, state_dim=A.shape[0], horizons=np.array(HORIZONS),
                   lens=np.array([len(t) for t in trajs]), obs=np.concatenate([t.obs for t in trajs]),
                   ctrls=np.concatenate([t.ctrls for t in trajs]), rmse=rmse)
        line = "%-14s %3d states  rmse %.3g .. %.3g  numpy composition vs reference %.1e" % (
            tag, A.shape[0], rmse[0], rmse[-1], np.max(np.abs(host / rmse - 1)))
        if with_rmsmens:
            model.pred_parallel = model.pred_batch
            out["rmsmens"] = np.array([G.quiet(get_model_rmsmens, model, trajs, horiz=h) for h in HORIZONS])
            assert np.all(np.isfinite(out["rmsmens"])), tag
            line += "  rmsmens %.3g .. %.3g" % (out["rmsmens"].min(), out["rmsmens"].max())
        print(line)
        G.save("kstep_wide_" + tag, **out)


if __name__ == "__main__":
    gen()
