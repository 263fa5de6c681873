"""fit_sindy_models(..., wide="device") (ONE ampc_sindy_fit_wide call for a batch's SINDy libraries of 273..2048 features:
csrc/sindyfit_wide_kernels.hpp) against the only path there was before it, the same models' train() in turn, for 64
configurations at CartPole shape (4 observations, 1 control) drawn from SINDyFactory's ranges by default_rng(0) (draws
whose library has at most 272 or more than 2048 features are drawn again) on 20 trajectories x 200 rows.  The two paths
alternate in one process after one warm-up each; the host clock runs around the call, which ends in a synchronise.
Also reported: how many configurations the device declined (status 1 pivot rule, status 2 threshold tie: those end in
train() inside the device path's time), and the device path's time by library width.
python tools/sindy_wide_fit_rate.py [repetitions] [--device-only]   (--device-only: the run rocprofv3 traces)"""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import SINDy, System                                                    # noqa: E402
from autompc_amd.sysid.sindy_fit import MAX_FEATURES, MAX_FEATURES_WIDE, fit_sindy_models   # noqa: E402
from autompc_amd import Trajectory                                                       # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = max(5, int(ARGS[0])) if ARGS else 5
DEVICE_ONLY = "--device-only" in sys.argv
N_MODELS, NO, NU = 64, 4, 1


def trajs(s, seed, n=100, L=200):
    """A damped nonlinear oscillator driven by random controls, scaled to |x| <= 0.8 (tools/sindy_fit_rate.py)."""
    no, nu = s.obs_dim, s.ctrl_dim
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(no, no))
    M = np.eye(no) + 0.1 * (-0.4 * np.eye(no) + 0.5 * (S - S.T) / np.sqrt(no / 3.0))
    G = rng.normal(scale=0.3, size=(no, nu))
    raw = []
    for _ in range(n):
        obs, ctl = np.zeros((L, no)), rng.uniform(-0.5, 0.5, size=(L, nu))
        x = rng.uniform(-0.5, 0.5, size=no)
        for i in range(L):
            obs[i] = x
            x = M @ x + 0.4 * np.sin(2.0 * x[::-1]) + G @ ctl[i]
        raw.append((obs, ctl))
    scale = 0.8 / max(np.max(np.abs(o)) for o, _ in raw)
    return [Trajectory(s, L, scale * o, c) for o, c in raw]


def sample_config(rng):
    """One draw from SINDyFactory's space (sysid/sindy.py: get_configuration_space)."""
    kw = dict(time_mode=str(rng.choice(["discrete", "continuous"])), poly_basis=bool(rng.integers(2)),
              trig_basis=bool(rng.integers(2)), threshold=float(10.0 ** rng.uniform(-5.0, 1.0)))
    if kw["poly_basis"]:
        kw.update(poly_degree=int(rng.integers(2, 9)), poly_cross_terms=bool(rng.integers(2)))
    if kw["trig_basis"]:
        kw.update(trig_freq=int(rng.integers(1, 9)), trig_interaction=bool(rng.integers(2)))
    return kw

system = System(["x%d" % i for i in range(NO)], ["u%d" % i for i in range(NU)], dt=0.05)
data = trajs(system, 1, n=20, L=200)
rng = np.random.default_rng(0)
kws, redrawn = [], 0
while len(kws) < N_MODELS:
    kw = sample_config(rng)
    if MAX_FEATURES < len(SINDy(system, **kw).library[0]) <= MAX_FEATURES_WIDE:
        kws.append(kw)
    else:
        redrawn += 1


def fresh():
    return [SINDy(system, **kw) for kw in kws]


def device_path():
    models = fresh()
    t0 = time.perf_counter()
    rep = fit_sindy_models(models, data, wide="device")
    return time.perf_counter() - t0, models, rep


def host_path():
    models = fresh()
    t0 = time.perf_counter()
    for m in models:
        m.train(data, silent=True)
    return time.perf_counter() - t0, models, None


feats = [len(m.library[0]) for m in fresh()]
print("%d SINDy configurations of %d .. %d features (median %d; %d draws outside %d .. %d drawn again), %d data rows"
      % (N_MODELS, min(feats), max(feats), int(statistics.median(feats)), redrawn, MAX_FEATURES + 1, MAX_FEATURES_WIDE,
         sum(len(t) for t in data)), flush=True)
PATHS = {"device": device_path} if DEVICE_ONLY else {"device": device_path, "train()": host_path}
times, last = {p: [] for p in PATHS}, {}
for p, run in PATHS.items():                                           # warm-up: kernels loaded, allocator primed
    run()
for _ in range(REPS):
    for p, run in PATHS.items():
        dt, models, rep = run()
        times[p].append(dt)
        last[p] = (models, rep)
rep = last["device"][1]
reasons = [r["reason"] for r in rep if r["where"] == "host"]
print("device path: %d Gram fits, %d train() calls (status 1: %d, status 2: %d, other: %d), %d designs"
      % (rep.device_fits, rep.host_fits, reasons.count("status 1"), reasons.count("status 2"),
         len([r for r in reasons if not r.startswith("status")]), rep.designs))
for p in PATHS:
    print("  %-8s median %.3f s (min %.3f, max %.3f) over %d repetitions"
          % (p, statistics.median(times[p]), min(times[p]), max(times[p]), REPS))
if not DEVICE_ONLY:
    print("  train() / device = %.2f" % (statistics.median(times["train()"]) / statistics.median(times["device"])))
    worst = 0.0
    for a, b, r in zip(last["device"][0], last["train()"][0], rep):
        if r["where"] == "device":
            den = max(float(np.max(np.abs(b.coefficients))), 1e-300)
            worst = max(worst, float(np.max(np.abs(a.coefficients - b.coefficients))) / den)
    print("  largest relative coefficient difference of the device-fitted models against train(): %.2e" % worst)
    # by width: the fitted (not declined) models of each third of the widths, each path alone on them
    order = np.argsort(feats)
    for part in np.array_split(order, 3):
        sub = [kws[i] for i in part]
        t = {}
        for p in ("device", "train()"):
            models = [SINDy(system, **kw) for kw in sub]
            t0 = time.perf_counter()
            if p == "device":
                fit_sindy_models(models, data, wide="device")
            else:
                for m in models:
                    m.train(data, silent=True)
            t[p] = time.perf_counter() - t0
        print("  %3d .. %4d features (%d configurations): device %.3f s, train() %.3f s, ratio %.2f"
              % (feats[part[0]], feats[part[-1]], len(part), t["device"], t["train()"], t["train()"] / t["device"]))
