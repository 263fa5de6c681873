"""model_errors(..., sindy_kstep="device") against the host loop over pred_batch (sindy_kstep="host", the only path
before ampc_kstep_errors_sindy) at CartPole shape (4 observations, 1 control, 100 trajectories x 200 steps) for 64
libraries drawn from SINDyFactory's ranges with random sparse coefficients: (a) horizons 1..10, (b) horizon 1 alone.
The two paths alternate in one process, one warm-up each, median of N timed calls, host clock around calls that end
in a synchronise, uploads included; the two score arrays must agree to 1e-9.
python tools/kstep_sindy_rate.py [calls] [--device-only]   (--device-only: the run rocprofv3 traces)"""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import SINDy, System, Trajectory                 # noqa: E402
from autompc_amd.evaluation import model_metrics as MM            # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
CALLS = int(ARGS[0]) if ARGS else 5
MODES = ("device",) if "--device-only" in sys.argv else ("host", "device")
NO, NU, N_MODELS = 4, 1, 64
s = System(["x%d" % i for i in range(NO)], ["u%d" % i for i in range(NU)], dt=0.05)


def trajs(seed, n=100, L=200):
    """A damped nonlinear oscillator driven by random controls, scaled to |x| <= 0.8 (powers up to x^8 stay small)."""
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(NO, NO))
    M = np.eye(NO) + 0.1 * (-0.4 * np.eye(NO) + 0.5 * (S - S.T))
    G = rng.normal(scale=0.1, size=(NO, NU))
    raw = []
    for _ in range(n):
        obs, ctl = np.zeros((L, NO)), rng.uniform(-0.5, 0.5, size=(L, NU))
        x = rng.uniform(-0.5, 0.5, size=NO)
        for i in range(L):
            obs[i] = x
            x = M @ x + 0.1 * np.sin(2.0 * x[::-1]) + G @ ctl[i]
        raw.append((obs, ctl))
    scale = 0.8 / max(np.max(np.abs(o)) for o, _ in raw)
    return [Trajectory(s, L, scale * o, c) for o, c in raw]


def sample_sindy(rng):
    """One draw from SINDyFactory's space (sysid/sindy.py: get_configuration_space) with coefficients instead of a
    fit: 0.9 (discrete) or -1 (continuous) on the identity part plus about six N(0, 0.05^2) terms per state."""
    kw = dict(time_mode=str(rng.choice(["discrete", "continuous"])), poly_basis=bool(rng.integers(2)),
              trig_basis=bool(rng.integers(2)))
    if kw["poly_basis"]:
        kw.update(poly_degree=int(rng.integers(2, 9)), poly_cross_terms=bool(rng.integers(2)))
    if kw["trig_basis"]:
        kw.update(trig_freq=int(rng.integers(1, 9)), trig_interaction=bool(rng.integers(2)))
    m = SINDy(s, **kw)
    nf = m.coefficients.shape[1]
    xi = (rng.random((NO, nf)) < min(0.15, 6.0 / nf)) * rng.normal(scale=0.05, size=(NO, nf))
    xi[:, :NO] += (-1.0 if kw["time_mode"] == "continuous" else 0.9) * np.eye(NO)
    m.set_coefficients(xi)
    return m


def compare(name, models, data, horizons):
    out, times, reports = {}, {m: [] for m in MODES}, {}
    for mode in MODES:                                            # warm-up: handles staged, kernels loaded
        MM.model_errors(models, data, horizons, "rmse", sindy_kstep=mode)
    for _ in range(CALLS):
        for mode in MODES:
            t0 = time.perf_counter()
            out[mode] = MM.model_errors(models, data, horizons, "rmse", sindy_kstep=mode)
            times[mode].append(time.perf_counter() - t0)
            reports[mode] = MM.last_report
    td = statistics.median(times["device"])
    line = "%-22s %2d models, %2d horizons | device median %7.4f s (min %.4f, max %.4f) | %d calls | %r" % (
        name, len(models), len(horizons), td, min(times["device"]), max(times["device"]), CALLS, reports["device"])
    assert reports["device"].host_fallbacks == 0 and reports["device"].sindy_calls == 1
    if "host" in MODES:
        th = statistics.median(times["host"])
        diff = float(np.max(np.abs(out["device"] / out["host"] - 1)))
        line += " | host median %8.3f s (min %.3f, max %.3f) | x%.0f | host fallbacks %d | max relative score " \
                "difference %.2e" % (th, min(times["host"]), max(times["host"]), th / td,
                                     reports["host"].host_fallbacks, diff)
        assert np.all(np.isfinite(out["host"])) and diff <= 1e-9, "the two paths disagree"
    print(line, flush=True)


test = trajs(2)
rng = np.random.default_rng(0)
models = [sample_sindy(rng) for _ in range(N_MODELS)]
sizes = [MM.sindy_program_sizes(m) for m in models]
print("%d SINDy models: features %d .. %d, %d with a product table (entries up to %d), %d evaluated directly, "
      "%d continuous" % (len(models), min(z[0] for z in sizes), max(z[0] for z in sizes),
                         sum(z[5] > 0 for z in sizes), max(z[5] for z in sizes), sum(z[5] == 0 for z in sizes),
                         sum(m.time_mode == "continuous" for m in models)), flush=True)
compare("(a) horizons 1..10", models, test, list(range(1, 11)))
compare("(b) horizon 1", models, test, [1])
