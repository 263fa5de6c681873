"""One Bayesian-optimisation proposal (tuning/proposer.py) on the device (ampc_bo_propose, csrc/bo_kernels.hpp) against
the numpy backend (gp_propose_host) and against the evaluate() of the batch it feeds, at the CartPole shape: MPPI
candidates of a 4-observation, 1-control system (d = 13), the default table (G = 24), q = 64 picks, n in {256, 1024,
2048} observations, pools of 8192 and 65536 points.  The observations are random candidates scored by a closed-loop-like
synthetic cost (so that the rank targets, the chosen row and the picks are those of a search in progress); the batch is
64 random MPPI candidates on the c1 workload (SINDy model, 49 control steps).  The three alternate in one process after
one warm-up each; the host clock runs around calls that end in a synchronise; medians of REPS repetitions.
python tools/bo_propose_rate.py [repetitions] [--device-only] [--no-numpy-above N] [--size N M]
  --device-only: the device proposal alone, the run rocprofv3 --kernel-trace --stats traces.
  --size N M: the one size n = N, pool = M instead of all six.
  --no-numpy-above N: skip the numpy backend where n > N (it takes tens of seconds at n = 2048)."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autompc_amd import _lib                                             # noqa: E402
from autompc_amd.synthetic import make_workload                          # noqa: E402
from autompc_amd.tuning import CandidateEvaluator, random_candidates     # noqa: E402
from autompc_amd.tuning.proposer import (CandidateEncoder, default_hypers, gp_propose_host,   # noqa: E402
                                         rank_targets)

def _option(name, count):
    """The `count` values behind option `name` (taken out of sys.argv), or None."""
    if name not in sys.argv:
        return None
    i = sys.argv.index(name)
    vals = [int(v) for v in sys.argv[i + 1:i + 1 + count]]
    del sys.argv[i:i + 1 + count]
    return vals


SIZE = _option("--size", 2)
NUMPY_CAP = (_option("--no-numpy-above", 1) or [1 << 30])[0]
DEVICE_ONLY = "--device-only" in sys.argv
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = max(5, int(ARGS[0])) if ARGS else 5
Q = 64

system, task, model, spec = make_workload("c1", precision="f64", device=0)
task.set_num_steps(50)
enc = CandidateEncoder(system, "mppi")
hw, hn = default_hypers(enc.d)
print("d = %d, G = %d, q = %d" % (enc.d, hw.shape[0], Q), flush=True)

batch = random_candidates(system, 64, seed=0)
for c in batch:
    c["Q"], c["R"], c["F"] = c["Q"] ** 0.25, c["R"] ** 0.25, c["F"] ** 0.25
ev = None if DEVICE_ONLY else CandidateEvaluator(system, task, model)


def observations(n, seed):
    rng = np.random.default_rng(seed)
    X = enc.snap(rng.random((n, enc.d)))
    centre, weight = np.linspace(0.25, 0.65, enc.d), np.linspace(2.0, 0.4, enc.d)
    scores = 10 ** (6.0 * np.sum(weight * (X - centre) ** 2, axis=1))
    scores[X[:, 0] > 0.8] = np.inf
    return X, rank_targets(scores)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


for m in ((SIZE[1],) if SIZE else (8192, 65536)):
    for n in ((SIZE[0],) if SIZE else (256, 1024, 2048)):
        X, z = observations(n, n)
        pool = enc.snap(np.random.default_rng(m + n).random((m, enc.d)))
        runs = {"device": lambda: _lib.bo_propose(X, z, hw, hn, pool, Q)}
        if not DEVICE_ONLY:
            if n <= NUMPY_CAP:
                runs["numpy"] = lambda: gp_propose_host(X, z, hw, hn, pool, Q)
            runs["evaluate"] = lambda: ev.evaluate(batch, seed=1)
        times, out = {k: [] for k in runs}, {}
        for k, fn in runs.items():                       # warm-up: kernels loaded, allocator primed
            out[k] = fn()
        for _ in range(REPS):                            # alternating
            for k, fn in runs.items():
                dt, _ = timed(fn)
                times[k].append(dt)
        med = {k: statistics.median(v) for k, v in times.items()}
        line = "n %4d  pool %5d: device %8.1f ms" % (n, m, 1e3 * med["device"])
        if "numpy" in med:
            same = int(np.sum(out["device"]["picks"] == out["numpy"]["picks"]))
            line += "  numpy %9.1f ms (%.1fx; same row %s, %d of %d picks equal)" % (
                1e3 * med["numpy"], med["numpy"] / med["device"], out["device"]["chosen"] == out["numpy"]["chosen"],
                same, Q)
        if "evaluate" in med:
            line += "  evaluate(64) %7.1f ms" % (1e3 * med["evaluate"])
        print(line + "  [row %d, lml %.1f]" % (out["device"]["chosen"], out["device"]["lml"][out["device"]["chosen"]]),
              flush=True)
