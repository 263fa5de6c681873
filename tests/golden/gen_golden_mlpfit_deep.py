#!/usr/bin/env python3
"""Golden vector of a deep sigmoid MLP fit, from the REAL reference (williamedwards/autompc).

Run in the build container only (needs the reference checkout that gen_golden.py installs):

    python tests/golden/gen_golden_mlpfit_deep.py

Writes ``tests/golden/mlpfit_p_sig4.npz`` (data only) with the fields of gen_golden.gen_mlpfit: the reference's own
``MLP(...).train(trajs)`` on its torch CPU path for FOUR hidden layers ``[17, 64, 15, 33]`` of sigmoid units, nx 4,
nu 2, ``n_batch`` 16 over 81 rows -- five full mini-batches and a ragged last batch of ONE row per epoch, three
epochs (18 optimiser steps).  The shapes sit on either side of the 16-wide tiles of the device fit
(csrc/mlpfit_kernels.hpp); tests/test_mlp_fit_device_host.py holds the torch fits to it, tests/test_gpu_mlp_fit_device.py
the device fit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G                                        # noqa: E402  (installs the reference)

G.MLPFIT_CASES = [("p_sig4", 4, 2, [17, 64, 15, 33], "sigmoid", 21, 3e-3, 3, 16, (3, 28))]

if __name__ == "__main__":
    G.gen_mlpfit()
    g = np.load(os.path.join(HERE, "mlpfit_p_sig4.npz"))
    rows = g["obs"].shape[0] * (g["obs"].shape[1] - 1)
    assert rows % int(g["n_batch"]) == 1, rows
    print("rows %d: %d full batches + 1 row, %d steps" % (rows, rows // 16, 3 * (rows // 16 + 1)))
