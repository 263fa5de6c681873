"""fit_linear_models(..., lasso="device") (one ampc_lasso_fit call per batch) against the same models' own train(), the
only path before it, at the HalfCheetah shape: 17 observations, 6 controls, 20 trajectories x 200 steps (3980 design
rows), 16 lasso configurations over four bases (x | x, x^2 | x, sin x, cos x | x, x^2, sin x, cos x: 23 .. 74
features) at alphas 1e-1, 1e-2, 1e-3, 1e-5.  Prints per path the wall time, and the largest coefficient difference.

python tools/lasso_fit_rate.py [calls] [--device-only]"""
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from autompc_amd import Koopman                                             # noqa: E402
from autompc_amd.sysid.linear_fit import fit_linear_models                  # noqa: E402
from linfit_cases import make_trajs, system                                 # noqa: E402

BASES = [dict(), dict(poly_basis=True, poly_degree=2), dict(trig_basis=True, trig_freq=1),
         dict(poly_basis=True, poly_degree=2, trig_basis=True, trig_freq=1)]
ALPHAS = [1e-1, 1e-2, 1e-3, 1e-5]


def models(s):
    return [Koopman(s, method="lasso", lasso_alpha=a, strict_reference=False, **b) for b in BASES for a in ALPHAS]


def main():
    calls = int(next((a for a in sys.argv[1:] if a.isdigit()), 3))
    s = system(17, 6)
    trajs = make_trajs(s, [200] * 20, 7)
    fit_linear_models(models(s), trajs, lasso="device")                      # warm-up: library load, allocations
    times = []
    for _ in range(calls):
        ms = models(s)
        t0 = time.perf_counter()
        rep = fit_linear_models(ms, trajs, lasso="device")
        times.append(time.perf_counter() - t0)
    print("device: %d configurations, median %.4f s (min %.4f, max %.4f) over %d calls; device fits %d, host fits %d, "
          "sweeps %s" % (len(ms), np.median(times), min(times), max(times), calls, rep.device_fits, rep.host_fits,
                         [r["sweeps"] for r in rep]), flush=True)
    print("where: %s" % [(r["where"], r["reason"]) for r in rep], flush=True)
    if "--device-only" in sys.argv:
        return
    ref = models(s)
    per = []
    Koopman(s, method="lasso", lasso_alpha=1.0).train(trajs[:2], silent=True)     # warm-up: sklearn's import
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for m in ref:
            t0 = time.perf_counter()
            m.train(trajs, silent=True)
            per.append(time.perf_counter() - t0)
            print("train() %2d: %.2f s" % (len(per), per[-1]), flush=True)
    err = max(float(np.max(np.abs(np.hstack([a.A, a.B]) - np.hstack([b.A, b.B]))) / np.max(np.abs(b.A)))
              for a, b, r in zip(ms, ref, rep) if r["where"] == "device")
    print("host train(): %.2f s for the batch (slowest model %.2f s); x%.0f; max relative coefficient difference %.2e"
          % (sum(per), max(per), sum(per) / np.median(times), err))


if __name__ == "__main__":
    main()
