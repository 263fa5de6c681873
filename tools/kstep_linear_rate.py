"""model_errors(..., linear_kstep="device") against the host loop over pred_batch (linear_kstep="host", the only
path before ampc_kstep_errors_linear) at HalfCheetah shape (17 observations, 6 controls, 100 trajectories x 200
steps): (a) ARX histories 4..10 at horizons 1..10, (b) 64 sampled ARX configurations (ARXFactory's range) at one
horizon, (c) Koopman lifts at one horizon.  The two paths alternate in one process, one warm-up each, median of N
timed calls, host clock around calls that end in a synchronise, uploads included; the two score arrays must agree
to 1e-9.  python tools/kstep_linear_rate.py [calls] [horizon of (b) and (c)]"""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import ARX, Koopman, System, Trajectory          # noqa: E402
from autompc_amd.evaluation import model_metrics as MM            # noqa: E402
from autompc_amd.sysid.linear_fit import fit_linear_models        # noqa: E402
from autompc_amd.tuning.configs import sample_arx_config          # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
HORIZON = int(sys.argv[2]) if len(sys.argv) > 2 else 1
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


def compare(name, models, data, horizons):
    out, times, reports = {}, {"host": [], "device": []}, {}
    for mode in ("host", "device"):                               # warm-up: handles staged, kernels loaded
        MM.model_errors(models, data, horizons, "rmse", linear_kstep=mode)
    for _ in range(CALLS):
        for mode in ("host", "device"):
            t0 = time.perf_counter()
            out[mode] = MM.model_errors(models, data, horizons, "rmse", linear_kstep=mode)
            times[mode].append(time.perf_counter() - t0)
            reports[mode] = MM.last_report
    diff = float(np.max(np.abs(out["device"] / out["host"] - 1)))
    th, td = statistics.median(times["host"]), statistics.median(times["device"])
    print("%-44s %2d models (%d wide), %2d horizons | host median %8.3f s (min %.3f, max %.3f) | device median "
          "%7.4f s (min %.4f, max %.4f) | x%.0f | %d calls each | host fallbacks %d -> %d | max relative score "
          "difference %.2e" % (name, len(models), reports["device"].wide_models, len(horizons), th,
                               min(times["host"]), max(times["host"]), td, min(times["device"]),
                               max(times["device"]), th / td, CALLS, reports["host"].host_fallbacks,
                               reports["device"].host_fallbacks, diff), flush=True)
    assert np.all(np.isfinite(out["host"])) and diff <= 1e-9, "the two paths disagree"
    assert reports["device"].host_fallbacks == 0


train, test = trajs(1), trajs(2)
rng = np.random.default_rng(0)
arx_a = [ARX(s, history=k) for k in range(4, 11)]
arx_b = [ARX(s, history=sample_arx_config(rng)["history"]) for _ in range(64)]
koop = {"identity": dict(), "poly 2": dict(poly_basis=True, poly_degree=2), "trig 1": dict(trig_basis=True),
        "x^2..x^4 + trig 1..3 (documented basis)": dict(poly_basis=True, poly_degree=4, trig_basis=True, trig_freq=3,
                                                        strict_reference=False),
        "x^2..x^3 + trig 1..2 (documented basis)": dict(poly_basis=True, poly_degree=3, trig_basis=True, trig_freq=2,
                                                        strict_reference=False),
        "trig 1..3 (documented basis)": dict(trig_basis=True, trig_freq=3, strict_reference=False)}
koop_c = [Koopman(s, **kw) for kw in koop.values()]
rep = fit_linear_models(arx_a + arx_b + koop_c, train)
print("fitted %d models (device fits %d, host fits %d); widths: ARX %s, Koopman %s"
      % (len(rep), rep.device_fits, rep.host_fits, sorted({m.A.shape[0] for m in arx_a + arx_b}),
         [m.A.shape[0] for m in koop_c]), flush=True)
compare("(a) ARX histories 4..10, horizons 1..10", arx_a, test, list(range(1, 11)))
compare("(b) 64 sampled ARX configurations, horizon %d" % HORIZON, arx_b, test, [HORIZON])
compare("(c) 6 Koopman lifts, horizon %d" % HORIZON, koop_c, test, [HORIZON])
