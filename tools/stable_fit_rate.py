"""fit_linear_models(..., stable="device") (one ampc_stable_fit call per batch) against sysid.stable_fit.stabilize_host,
the reference's routine restated on the data, at the HalfCheetah shape: 17 observations, 6 controls, 20 trajectories
x 200 steps (3980 design rows), the three distinct bases with at most 64 lifted states (x | x, x^2 | x, sin x, cos x:
n = 17, 34, 51).  The data are stablefit_cases.make_data's (a slightly unstable rotation, rho 1.002).

Prints the device call end to end (median of five), ampc_stable_fit alone on the three bases replicated 1, 4, 16 and
64 times (every configuration of a call has its own workgroup: what a batch costs), stabilize_host per basis with the
process pinned to 16 CPUs, and the largest coefficient difference.  --device-only stops after the device call and
prints its trial count: run under ``rocprofv3 --kernel-trace --stats`` it gives stable_fgm_kernel's own time per trial.

python tools/stable_fit_rate.py [--device-only]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from autompc_amd import Koopman, Trajectory, _lib                           # noqa: E402
from autompc_amd.sysid.linear_fit import concat_trajs, fit_linear_models    # noqa: E402
from autompc_amd.sysid.stable_fit import koopman_rows, stabilize_host       # noqa: E402
from linfit_cases import system                                             # noqa: E402
from stablefit_cases import make_data                                       # noqa: E402

BASES = [dict(), dict(poly_basis=True, poly_degree=2), dict(trig_basis=True, trig_freq=1)]
DATA = dict(no=17, nu=6, lengths=[200] * 20, seed=7, rho=1.002, amp=0.5)


def models(s):
    return [Koopman(s, method="stable", strict_reference=False, **b) for b in BASES]


def main():
    s = system(17, 6)
    lens, obs, ctrls = make_data(DATA)
    trajs, r = [], 0
    for n in lens:
        trajs.append(Trajectory(s, int(n), obs[r:r + n].copy(), ctrls[r:r + n].copy()))
        r += int(n)
    fit_linear_models(models(s), trajs, stable="device")                     # warm-up: library load, allocations
    times = []
    for _ in range(5):
        ms = models(s)
        t0 = time.perf_counter()
        rep = fit_linear_models(ms, trajs, stable="device")
        times.append(time.perf_counter() - t0)
    trials = [r.get("trials") for r in rep]
    print("device: %d bases (n = %s), median %.4f s (min %.4f, max %.4f) over 5 calls; where %s; iterations %s, "
          "trials %s (total %d)" % (len(ms), [m.state_dim for m in ms], np.median(times), min(times), max(times),
                                    [(r["where"], r["reason"]) for r in rep], [r.get("iterations") for r in rep],
                                    trials, sum(t or 0 for t in trials)), flush=True)
    if "--device-only" in sys.argv:
        return
    cl, co, cc = concat_trajs(trajs)
    lifts = [m.device_lift() for m in ms]
    for k in (1, 4, 16, 64):
        per = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = _lib.stable_fit(cl, co, cc, lifts * k)
            per.append(time.perf_counter() - t0)
        print("ampc_stable_fit: %3d configurations (the 3 bases x %2d) median %.4f s of 3, %.4f s per configuration; "
              "status %s" % (3 * k, k, np.median(per), np.median(per) / (3 * k), sorted(set(out[1].tolist()))),
              flush=True)
    cpus = sorted(os.sched_getaffinity(0))[:16]
    os.sched_setaffinity(0, cpus)
    host, err = [], 0.0
    for m in ms:
        rows = koopman_rows(cl, co, cc, m.device_lift())
        best = []
        for _ in range(3):
            st = {}
            t0 = time.perf_counter()
            A, B, _ = stabilize_host(*rows, stats=st)
            best.append(time.perf_counter() - t0)
        host.append(np.median(best))
        if m.A is not None:
            err = max(err, float(np.max(np.abs(np.hstack([A, B]) - np.hstack([m.A, m.B]))) / np.max(np.abs(A))))
        print("stabilize_host n = %2d: median %.3f s of 3 (%d CPUs), trials %d" % (m.state_dim, host[-1], len(cpus),
                                                                                  st["trials"]), flush=True)
    print("host: %.3f s for the three bases; device call x%.2f of that; max relative coefficient difference %.2e"
          % (sum(host), np.median(times) / sum(host), err))


if __name__ == "__main__":
    main()
