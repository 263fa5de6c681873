"""fit_linear_models against the train() loop at HalfCheetah shape (17 observations, 6 controls, 100 trajectories x
200 steps): the ten ARX histories and 64 sampled ARX configurations (ARXFactory's range), uploads and host fits
included, median of N calls after one warm-up; plus the coefficient difference between the two.
python tools/linfit_rate.py [calls]"""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import ARX, Koopman, System, Trajectory          # noqa: E402
from autompc_amd.sysid.linear_fit import fit_linear_models        # noqa: E402
from autompc_amd.tuning.configs import sample_arx_config          # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
NO, NU = 17, 6
s = System(["x%d" % i for i in range(NO)], ["u%d" % i for i in range(NU)], dt=0.05)


def trajs(seed, n=100, L=200):
    """A damped nonlinear oscillator driven by random controls."""
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(NO, NO))
    M = np.eye(NO) + 0.1 * (-0.4 * np.eye(NO) + 0.5 * (S - S.T) / np.sqrt(NO / 3.0))
    G = rng.normal(scale=0.3, size=(NO, NU))
    out = []
    for _ in range(n):
        obs, ctl = np.zeros((L, NO)), rng.uniform(-1.0, 1.0, size=(L, NU))
        x = rng.uniform(-1.0, 1.0, size=NO)
        for i in range(L):
            obs[i] = x
            x = M @ x + 0.4 * np.sin(2.0 * x[::-1]) + G @ ctl[i]
        out.append(Trajectory(s, L, obs, ctl))
    return out


def median_time(fn, calls):
    fn()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


data = trajs(1)
rng = np.random.default_rng(0)
sets = {"ARX histories 1..10": list(range(1, 11)),
        "64 sampled ARX configurations": [sample_arx_config(rng)["history"] for _ in range(64)]}
for name, hist in sets.items():
    host_models = [ARX(s, history=k) for k in hist]
    t0 = time.perf_counter()
    for m in host_models:                                         # the parent commit's path: one SVD solve per column
        m.train(data)
    t_host = time.perf_counter() - t0
    dev_models = [ARX(s, history=k) for k in hist]
    reports = []
    med, lo, hi = median_time(lambda: reports.append(fit_linear_models(dev_models, data)), CALLS)
    rep = reports[-1]
    err = max(np.abs(a.coeffs - b.coeffs).max() / np.abs(a.coeffs).max() for a, b in zip(host_models, dev_models))
    print("%-32s train() loop %7.2f s (one pass) | fit_linear_models median %.4f s (min %.4f, max %.4f, %d calls) | "
          "x%.0f | device fits %d, host fits %d | min pivot %.2e | max coefficient difference %.2e"
          % (name, t_host, med, lo, hi, CALLS, t_host / med, rep.device_fits, rep.host_fits,
             min(r["pivot"] for r in rep), err), flush=True)

koop = {"identity": dict(), "poly 2": dict(poly_basis=True, poly_degree=2), "trig 1": dict(trig_basis=True),
        "x^2..x^4 + trig 1..3 (documented basis)": dict(poly_basis=True, poly_degree=4, trig_basis=True, trig_freq=3,
                                                        strict_reference=False)}
host_models = [Koopman(s, **kw) for kw in koop.values()]
t0 = time.perf_counter()
for m in host_models:
    m.train(data)
t_host = time.perf_counter() - t0
dev_models = [Koopman(s, **kw) for kw in koop.values()]
reports = []
med, lo, hi = median_time(lambda: reports.append(fit_linear_models(dev_models, data)), CALLS)
print("%-32s train() loop %7.2f s | fit_linear_models median %.4f s (min %.4f, max %.4f)"
      % ("4 Koopman lifts (17..170 states)", t_host, med, lo, hi))
for name, a, b, r in zip(koop, host_models, dev_models, reports[-1]):
    print("    %-42s %-6s pivot %.2e  max |A, B| difference %.2e"
          % (name, r["where"], r["pivot"], max(np.abs(a.A - b.A).max(), np.abs(a.B - b.B).max()) / np.abs(a.A).max()))
