"""A Bayesian-optimisation proposer for the batch tuner: GP surrogate, batch expected improvement.

What it replaces.  The reference drives ``PipelineTuner`` with SMAC (autompc/tuning/pipeline_tuner.py:151-319), a
model-based optimiser that learns from every ``eval_cfg`` result where the next configuration should go and
interleaves random configurations with its own.  ``BatchPipelineTuner`` proposed by random search only.  A
``GpProposer`` passed as ``BatchPipelineTuner(..., proposer=...)`` sees every batch's surrogate scores (``observe``)
and proposes the next batch from them.  SMAC's surrogate is a random forest and proposes one configuration at a time;
this one is a Gaussian process that proposes a whole batch, so that the proposal is dense linear algebra: the hot path
is ``ampc_bo_propose`` (csrc/bo_kernels.hpp) on the device, ``gp_propose_host`` below is the same algorithm in numpy
(``backend="numpy"``; no scipy, no GPU).

The algorithm.  All arithmetic is f64.

1. Encoding (``CandidateEncoder``).  A candidate dict is a point of [0, 1]^d and back.  ``kind="mppi"``: horizon (int
   5..30), sigma (1e-4..2), lmda (0.1..2), num_path (int 100..1000), all linear, then the Q, R, F diagonals as log10
   over [-3, 4] -- the ranges of ``random_candidates``.  ``kind="ilqr"``: horizon (int 5..25), then the three diagonals
   -- ``random_ilqr_candidates``.  With ``models=[...]`` a one-hot block for ``model_index`` is appended (decode: the
   largest entry, lowest index on ties; it sets ``model`` and ``model_index``).  ``decode`` clips to the range and
   rounds integer axes.  Pool points are snapped (``encode(decode(p))``) before the GP sees them: the surrogate is
   evaluated at configurations that can run.

2. Targets (``rank_targets``).  Scores that are not finite count as +inf; the scores are ranked 1..n with average
   ranks for ties; z = Phi^-1((rank - 0.5) / n) (``statistics.NormalDist().inv_cdf``).

3. Surrogate.  A zero-mean GP with the Matern-5/2 kernel of unit signal variance, k(a, b) = (1 + s + s^2 / 3) exp(-s),
   s = sqrt(5) |(a - b) o w|, w the per-dimension inverse length scales; the squared distance is summed directly over
   the dimensions (the expansion |a|^2 + |b|^2 - 2 a.b cancels).  A hyperparameter table of G rows (w [d], noise); the
   default (``default_hypers``) is isotropic, w = 1 / (l sqrt d) for l in {0.1, 0.2, 0.4, 0.8, 1.6, 3.2} times noise
   in {1e-6, 1e-4, 1e-2, 1e-1} (l outer, noise inner: G = 24).  Per row K = k(X, X) + noise I = L L', L t = z,
   lml = -t't / 2 - sum log L_ii.  A row whose factorisation meets a pivot that is not positive and finite is declined
   (status 1, lml -inf).  The chosen row is the accepted row of largest lml, lowest index on ties.

4. Pool posterior.  For the M snapped pool points P: V = L^-1 k(X, P) ([n][M]), mu = V't, sigma^2 = max(1 - colsum V^2,
   VAR_FLOOR).  Expected improvement for minimisation against z_min = min z: u = (z_min - mu) / sigma,
   EI = sigma (u Phi(u) + phi(u)), Phi(u) = erfc(-u / sqrt 2) / 2.

5. Greedy batch picks with the "believer" update.  For pick t = 0 .. q' - 1: j_t = argmax EI over the points not yet
   picked (lowest index on ties; a NaN EI counts as -inf); the posterior covariance of every pool point with the pick,
   c = k(P, p_j) - V'V[:, j] - sum_{s<t} r_s r_s[j]; the new row r_t = c / sqrt(max(c[j] + noise, VAR_FLOOR));
   sigma^2 <- max(sigma^2 - r_t^2, VAR_FLOOR); the mean stays (the pick is believed to score its mean) and EI is
   recomputed.  This appends a row to V per pick and equals refitting the GP on n + t + 1 points.  Per pick its EI and
   the margin (EI_best - EI_second) / EI_best are reported (EI_second = 0 when the pick was the last unpicked point;
   margin 0 when EI_best <= 0).

6. The proposer (``GpProposer``).  Until ``n_init`` observations exist (default: the first batch's size) a batch is
   random, from the draw functions ``BatchPipelineTuner._random_search`` uses.  Afterwards ceil(random_fraction n) of
   the batch stays random (SMAC interleaves random configurations the same way) and the rest are picks.  The pool is
   half uniform draws, half Gaussian perturbations (sigma 0.05, clipped) of the eight best observed points.  Every
   random number comes from the ``rng`` passed in.  When the history exceeds ``max_points`` the GP is fitted on the
   max_points / 2 lowest scores (earlier index on ties) plus the most recent of the remainder.  If every
   hyperparameter row is declined the batch is random and ``declined_batches`` counts it.  ``last`` says what happened.
"""
import math
from statistics import NormalDist

import numpy as np

VAR_FLOOR = 1e-12          # (kBoVarFloor of csrc/bo_kernels.hpp)
LENGTH_SCALES = (0.1, 0.2, 0.4, 0.8, 1.6, 3.2)
NOISES = (1e-6, 1e-4, 1e-2, 1e-1)
# the limits of ampc_bo_propose
MAX_N, MAX_D, MAX_G, MAX_M, MAX_Q = 2048, 64, 64, 65536, 256

_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def default_hypers(d):
    """The default table: (w [24][d], noise [24]), length scale outer, noise inner."""
    w = [np.full(d, 1.0 / (l * math.sqrt(d))) for l in LENGTH_SCALES for _ in NOISES]
    noise = [s for _ in LENGTH_SCALES for s in NOISES]
    return np.array(w, dtype=np.float64), np.array(noise, dtype=np.float64)


class CandidateEncoder:
    """Candidate dict <-> point of [0, 1]^d (step 1 of the module docstring)."""
    LOG_LO, LOG_HI = -3.0, 4.0

    def __init__(self, system, kind, models=None):
        if kind not in ("mppi", "ilqr"):
            raise ValueError("kind must be 'mppi' or 'ilqr'")
        self.system, self.kind = system, kind
        self.models = list(models) if models else None
        self.no, self.nu = system.obs_dim, system.ctrl_dim
        if kind == "mppi":      # (key, lo, hi, integer)
            self.scalars = [("horizon", 5.0, 30.0, True), ("sigma", 1e-4, 2.0, False), ("lmda", 0.1, 2.0, False),
                            ("num_path", 100.0, 1000.0, True)]
        else:
            self.scalars = [("horizon", 5.0, 25.0, True)]
        self.n_gain = 2 * self.no + self.nu
        self.n_model = len(self.models) if self.models else 0
        self.d = len(self.scalars) + self.n_gain + self.n_model

    def encode(self, cand):
        x = np.empty(self.d)
        k = 0
        for key, lo, hi, _ in self.scalars:
            x[k] = (float(cand[key]) - lo) / (hi - lo)
            k += 1
        for key, width in (("Q", self.no), ("R", self.nu), ("F", self.no)):
            g = np.asarray(cand[key], dtype=np.float64)
            if g.ndim == 2:
                g = np.diag(g)
            x[k:k + width] = (np.log10(g) - self.LOG_LO) / (self.LOG_HI - self.LOG_LO)
            k += width
        if self.n_model:
            idx = cand.get("model_index")
            if idx is None:                     # (a candidate that names its model only)
                idx = next(i for i, m in enumerate(self.models) if m is cand["model"])
            x[k:] = 0.0
            x[k + int(idx)] = 1.0
        return np.clip(x, 0.0, 1.0)

    def decode(self, x):
        x = np.clip(np.asarray(x, dtype=np.float64), 0.0, 1.0)
        cand = {}
        k = 0
        for key, lo, hi, integer in self.scalars:
            v = lo + x[k] * (hi - lo)
            cand[key] = int(min(max(round(v), lo), hi)) if integer else float(min(max(v, lo), hi))
            k += 1
        for key, width in (("Q", self.no), ("R", self.nu), ("F", self.no)):
            cand[key] = 10.0 ** (self.LOG_LO + x[k:k + width] * (self.LOG_HI - self.LOG_LO))
            k += width
        if self.n_model:
            idx = int(np.argmax(x[k:]))
            cand["model"], cand["model_index"] = self.models[idx], idx
        return cand

    def snap(self, P):
        """``encode(decode(p))`` of every row of P, without going through dicts: integer axes to their grid, the model
        block to its one-hot corner; the continuous axes are clipped."""
        P = np.clip(np.array(P, dtype=np.float64, ndmin=2), 0.0, 1.0)
        for k, (_, lo, hi, integer) in enumerate(self.scalars):
            if integer:
                P[:, k] = (np.clip(np.round(lo + P[:, k] * (hi - lo)), lo, hi) - lo) / (hi - lo)
        if self.n_model:
            k = self.d - self.n_model
            idx = np.argmax(P[:, k:], axis=1)
            P[:, k:] = 0.0
            P[np.arange(P.shape[0]), k + idx] = 1.0
        return P


def rank_targets(scores):
    """Step 2: scores -> z (non-finite scores rank last, ties share their average rank)."""
    s = np.array(scores, dtype=np.float64).ravel()
    s[~np.isfinite(s)] = np.inf
    n = s.shape[0]
    order = np.argsort(s, kind="stable")
    rank = np.empty(n)
    i = 0
    while i < n:
        j = i
        while j + 1 < n and s[order[j + 1]] == s[order[i]]:
            j += 1
        rank[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    inv = NormalDist().inv_cdf
    return np.array([inv((r - 0.5) / n) for r in rank])


def matern52(A, B, w):
    """k(A, B) [na][nb], the squared distance summed over the dimensions in order."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    s2 = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        t = (A[:, k, None] - B[None, :, k]) * w[k]
        s2 += t * t
    s = math.sqrt(5.0) * np.sqrt(s2)
    return (1.0 + s + s * s / 3.0) * np.exp(-s)


def expected_improvement(mu, var, zmin):
    sd = np.sqrt(var)
    u = (zmin - mu) / sd
    Phi = 0.5 * _erfc(-u * math.sqrt(0.5))
    phi = np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return sd * (u * Phi + phi)


def _check_sizes(n, d, G, m, q):
    if not 1 <= n <= MAX_N:
        raise ValueError("n (observations) must be in 1..%d" % MAX_N)
    if not 1 <= d <= MAX_D:
        raise ValueError("d (dimensions) must be in 1..%d" % MAX_D)
    if not 1 <= G <= MAX_G:
        raise ValueError("the hyperparameter table must have 1..%d rows" % MAX_G)
    if not 1 <= m <= MAX_M:
        raise ValueError("m (pool points) must be in 1..%d" % MAX_M)
    if not 1 <= q <= min(m, MAX_Q):
        raise ValueError("q (picks) must be in 1..min(m, %d)" % MAX_Q)


def gp_propose_host(X, z, hyper_w, hyper_noise, pool, q, full=False):
    """Steps 3-5 in numpy; the same arguments, limits and result dict as ``_lib.bo_propose``.  full: the believer
    update is also made after the last pick and the dict carries "var_picks" [q][m], sigma^2 after each pick."""
    X, pool = np.asarray(X, dtype=np.float64), np.asarray(pool, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64).ravel()
    hw, hn = np.asarray(hyper_w, dtype=np.float64), np.asarray(hyper_noise, dtype=np.float64).ravel()
    n, d = X.shape
    m, G, q = pool.shape[0], hw.shape[0], int(q)
    _check_sizes(n, d, G, m, q)
    lml, status = np.full(G, -np.inf), np.zeros(G, dtype=np.int32)
    best, best_L, best_t = -1, None, None
    for g in range(G):
        K = matern52(X, X, hw[g])
        K[np.diag_indices(n)] += hn[g]
        try:
            L = np.linalg.cholesky(K)
        except np.linalg.LinAlgError:
            L = None
        if L is None or not np.all(np.isfinite(L)) or not np.all(np.diag(L) > 0.0):
            status[g] = 1
            continue
        t = np.linalg.solve(L, z)
        lml[g] = -0.5 * float(t @ t) - float(np.sum(np.log(np.diag(L))))
        if not np.isfinite(lml[g]):
            status[g], lml[g] = 1, -np.inf
            continue
        if best < 0 or lml[g] > lml[best]:
            best, best_L, best_t = g, L, t
    out = dict(lml=lml, status=status, chosen=best, picks=np.full(q, -1, dtype=np.int32),
               pick_ei=np.full(q, np.nan), pick_margin=np.full(q, np.nan), mu=np.full(m, np.nan),
               var=np.full(m, np.nan))
    if best < 0:
        return out
    w, noise, zmin = hw[best], float(hn[best]), float(z.min())
    V = np.linalg.solve(best_L, matern52(X, pool, w))
    mu = V.T @ best_t
    var = np.maximum(1.0 - np.sum(V * V, axis=0), VAR_FLOOR)
    out["mu"], out["var"] = mu, var.copy()
    ei = expected_improvement(mu, var, zmin)
    picked = np.zeros(m, dtype=bool)
    rows = []
    for step in range(q):
        cand = np.where(np.isnan(ei), -np.inf, ei)
        free = np.flatnonzero(~picked)          # (an unpicked point of EI -inf still beats every picked one)
        j = int(free[np.argmax(cand[free])])
        bestv = float(cand[j])
        rest = free[free != j]
        second = float(np.max(cand[rest])) if rest.size else 0.0
        out["picks"][step], out["pick_ei"][step] = j, bestv
        out["pick_margin"][step] = (bestv - second) / bestv if bestv > 0.0 else 0.0
        picked[j] = True
        if step + 1 == q and not full:
            break
        c = matern52(pool, pool[j:j + 1], w)[:, 0] - V.T @ V[:, j]
        for r in rows:
            c -= r * r[j]
        r = c / math.sqrt(max(c[j] + noise, VAR_FLOOR))
        rows.append(r)
        var = np.maximum(var - r * r, VAR_FLOOR)
        if full:
            out.setdefault("var_picks", []).append(var.copy())
        ei = expected_improvement(mu, var, zmin)
    if full:
        out["var_picks"] = np.array(out["var_picks"])
    return out


class GpProposer:
    """``proposer(n, rng) -> n candidates``; ``proposer.observe(candidates, scores)`` (step 6 of the module docstring).
    backend: "device" (``ampc_bo_propose``) or "numpy" (``gp_propose_host``).  hypers: (w [G][d], noise [G]) or None
    for ``default_hypers``.  last: {"path": "random" | "gp" | "declined", "n", "chosen", "lml", "min_margin",
    "picks", "pick_ei", "pick_margin"} of the latest batch."""

    def __init__(self, system, kind, models=None, backend="device", pool=8192, random_fraction=0.25, n_init=None,
                 max_points=1024, hypers=None, device=0):
        if backend not in ("device", "numpy"):
            raise ValueError("backend must be 'device' or 'numpy'")
        self.encoder = CandidateEncoder(system, kind, models)
        self.system, self.kind, self.models = system, kind, self.encoder.models
        self.backend, self.device = backend, int(device)
        self.pool = int(pool)
        self.random_fraction = float(random_fraction)
        self.n_init = None if n_init is None else int(n_init)
        self.max_points = int(max_points)
        if not 2 <= self.max_points <= MAX_N:
            raise ValueError("max_points must be in 2..%d" % MAX_N)
        if not 2 <= self.pool <= MAX_M:
            raise ValueError("pool must be in 2..%d" % MAX_M)
        if not 0.0 <= self.random_fraction <= 1.0:
            raise ValueError("random_fraction must be in [0, 1]")
        if self.encoder.d > MAX_D:
            raise ValueError("the encoded space has %d dimensions, the limit is %d" % (self.encoder.d, MAX_D))
        if hypers is None:
            hypers = default_hypers(self.encoder.d)
        self.hyper_w = np.ascontiguousarray(hypers[0], dtype=np.float64)
        self.hyper_noise = np.ascontiguousarray(hypers[1], dtype=np.float64).ravel()
        if self.hyper_w.ndim != 2 or self.hyper_w.shape != (self.hyper_noise.shape[0], self.encoder.d):
            raise ValueError("hypers must be (w [G][%d], noise [G])" % self.encoder.d)
        self.X, self.scores = [], []
        self.declined_batches = 0
        self.last = None

    # -- history ------------------------------------------------------------------------------------------
    def observe(self, candidates, scores):
        scores = np.asarray(scores, dtype=np.float64).ravel()
        if len(candidates) != scores.shape[0]:
            raise ValueError("one score per candidate expected")
        for c, s in zip(candidates, scores):
            self.X.append(self.encoder.encode(c))
            self.scores.append(float(s) if np.isfinite(s) else float("inf"))

    def _fit_set(self):
        """Indices of the history the GP is fitted on, ascending."""
        n = len(self.scores)
        if n <= self.max_points:
            return np.arange(n)
        s = np.asarray(self.scores)
        keep = np.argsort(s, kind="stable")[:self.max_points // 2]
        rest = np.setdiff1d(np.arange(n), keep)
        return np.sort(np.concatenate([keep, rest[-(self.max_points - keep.shape[0]):]]))

    # -- proposals ----------------------------------------------------------------------------------------
    def _random(self, n, rng):
        from .batch_eval import random_candidates, random_ilqr_candidates
        draw = random_candidates if self.kind == "mppi" else random_ilqr_candidates
        cands = draw(self.system, n, seed=int(rng.integers(1 << 31)))
        if self.models:
            for c, k in zip(cands, rng.integers(len(self.models), size=n)):
                c["model"], c["model_index"] = self.models[int(k)], int(k)
        return cands

    def _pool(self, X, scores, rng):
        d = self.encoder.d
        n_uni = self.pool // 2
        uni = rng.random((n_uni, d))
        top = X[np.argsort(scores, kind="stable")[:8]]
        n_loc = self.pool - n_uni
        centre = top[np.arange(n_loc) % top.shape[0]]
        loc = np.clip(centre + rng.normal(0.0, 0.05, size=(n_loc, d)), 0.0, 1.0)
        return self.encoder.snap(np.concatenate([uni, loc]))

    def propose(self, X, z, pool, q):
        if self.backend == "device":
            from .. import _lib
            return _lib.bo_propose(X, z, self.hyper_w, self.hyper_noise, pool, q, device=self.device)
        return gp_propose_host(X, z, self.hyper_w, self.hyper_noise, pool, q)

    def __call__(self, n, rng):
        n = int(n)
        if self.n_init is None:
            self.n_init = n
        n_rand = min(n, int(math.ceil(self.random_fraction * n)))
        q = n - n_rand
        if len(self.scores) < max(self.n_init, 1) or q < 1:
            self.last = dict(path="random", n=len(self.scores), chosen=None, lml=None, min_margin=None)
            return self._random(n, rng)
        if q > min(MAX_Q, self.pool):
            raise ValueError("a batch may hold at most min(pool, %d) picks" % MAX_Q)
        idx = self._fit_set()
        X = np.array([self.X[i] for i in idx])
        scores = np.array([self.scores[i] for i in idx])
        z = rank_targets(scores)
        pool = self._pool(X, scores, rng)
        res = self.propose(X, z, pool, q)
        if res["chosen"] < 0:
            self.declined_batches += 1
            self.last = dict(path="declined", n=len(idx), chosen=None, lml=None, min_margin=None)
            return self._random(n, rng)
        self.last = dict(path="gp", n=len(idx), chosen=int(res["chosen"]), lml=float(res["lml"][res["chosen"]]),
                         min_margin=float(np.min(res["pick_margin"])), picks=np.array(res["picks"]),
                         pick_ei=np.array(res["pick_ei"]), pick_margin=np.array(res["pick_margin"]))
        cands = [self.encoder.decode(pool[int(j)]) for j in res["picks"]]
        return cands + self._random(n_rand, rng)
