"""Batched fits of SINDy models: one Gram pass per feature library, thresholded solves on its sub-matrices.

``SINDy.train`` is a sequentially-thresholded least squares (STLSQ): per target column and iteration it solves the
ridge normal equations ``(A'A + alpha I) w = A'y`` on the kept columns ``A`` of the design matrix ``Theta`` and drops
the columns with ``|w| < threshold``, re-forming ``A'A`` over all data rows every time.  Every one of those systems is
a sub-matrix of ONE Gram matrix ``Theta'[Theta | Y]`` of the model's feature library, so a tuner's batch of SINDy
configurations of one data set needs one Gram per distinct library (a "design") and then only small solves.
``fit_sindy_models`` forms the Grams of all designs on the device in one launch (``ampc_sindy_fit``: design rows built
on the fly, f64 MFMA, fixed-order sums) and solves every (configuration, target) there: gather, scale to unit
diagonal, Cholesky, threshold, repeat.  A configuration is (library, time mode, threshold); ``alpha`` and
``max_iter`` belong to the call.  ``method`` and ``lasso_alpha`` do not enter: ``train()`` ignores them.

When the device declines.  Status 1: §6d's pivot rule failed in some solve of some target (a non-positive or
non-finite diagonal entry or pivot, a non-finite coefficient, or a smallest squared pivot of the unit-diagonal matrix
below ``n_kept * 2^-26``).  Status 2, a threshold tie: some kept coefficient of some solve lies within a relative
``2^-20`` of the threshold.  With the pivot rule passed a coefficient carries at most about ``2^-27`` relative error
(``eps / sqrt(eps)``); ``2^-20`` leaves a factor 100 over that.  A coefficient this close to the threshold could be
kept on one path and dropped on the other, and the two fits would then differ by a whole feature.  Either way the
model is fitted by its own ``train()``, as are models over the device limits (272 features, 64 states, 16 controls:
"size"), subclasses that override ``train`` ("subclass"), and continuous-mode models whose data hold a trajectory
shorter than 2 rows without ``xdot`` (``np.gradient`` raises for it in ``train()``; it is left to raise).  Every
model ends up exactly as after its own ``train(trajs, xdot=xdot, alpha=alpha, max_iter=max_iter)``, through
``set_coefficients``.

``stlsq_gram_host`` is the same algorithm in numpy (what the CPU tests run and the GPU tests compare against first).

Libraries of 273..2048 features (``wide="device"``, opt-in).  The same algorithm on a second pair of kernels
(``ampc_sindy_fit_wide``: the design rows of a run of 512-row splits materialised once, a rank-k MFMA pass that sums
the splits in order, a Cholesky blocked by 32 columns whose trailing update runs on the matrix pipe; Gram pass and
solves in waves under a memory budget).  A batch's models of at most 272 features keep the narrow call, the wider ones
make one wide call; statuses 1 and 2 and libraries over 2048 features end in ``train()`` as before.
"""
import numpy as np

from .. import _lib
from .linear_fit import PIVOT_EPS, SPLIT_ROWS, _row_start, concat_trajs
from .sindy import SINDy, _features

MAX_FEATURES, MAX_STATE, MAX_CTRL = 272, 64, 16
MAX_FEATURES_WIDE = 2048               # with wide="device": libraries of 273..2048 features take ampc_sindy_fit_wide
TIE_MARGIN = 2.0 ** -20                # relative distance of a coefficient to the threshold below which a fit is a tie


def design_gram(lens, obs, ctrls, lib, ycont=None):
    """G = Theta'[Theta | Y_discrete | Y_continuous] of one library over the rows with a successor, summed over
    blocks of SPLIT_ROWS data rows in order (the blocks are the device's row splits).  Y_continuous only when
    `ycont` is given."""
    _, valid = _row_start(lens)
    V = np.concatenate([obs, ctrls], axis=1)
    nf = len(lib[0])
    nt = obs.shape[1] * (2 if ycont is not None else 1)
    G = np.zeros((nf, nf + nt))
    for r0 in range(0, obs.shape[0], SPLIT_ROWS):
        g = r0 + np.nonzero(valid[r0:r0 + SPLIT_ROWS])[0]
        if not len(g):
            continue
        Th = _features(lib, V[g])
        cols = [Th, obs[g + 1]] + ([ycont[g]] if ycont is not None else [])
        G += Th.T @ np.concatenate(cols, axis=1)
    return G


def _scaled_cholesky_1(S, b):
    """Solve S w = b for symmetric positive definite S by D S D with D = diag(S)^-1/2 and a right-looking Cholesky,
    the right-hand side carried as an extra row.  Returns (w or None, smallest squared pivot)."""
    n = len(b)
    diag = np.diag(S)
    if not (np.all(diag > 0) and np.all(np.isfinite(diag))):
        return None, float(np.min(diag))
    d = 1.0 / np.sqrt(diag)
    M = np.empty((n + 1, n))
    M[:n] = S * d[:, None] * d[None, :]
    M[n] = b * d
    minp = np.inf
    for j in range(n):
        p = M[j, j]
        if not (p > 0 and np.isfinite(p)):
            return None, float(p)
        minp = min(minp, p)
        M[j, j] = np.sqrt(p)
        M[j + 1:, j] /= M[j, j]
        M[j + 1:, j + 1:] -= np.multiply.outer(M[j + 1:, j], M[j + 1:n, j])
    y = M[n]
    for j in range(n - 1, -1, -1):
        y[j] /= M[j, j]
        y[:j] -= y[j] * M[j, :j]
    return y * d, float(minp)


def stlsq_gram(G, nf, tcol, threshold, alpha, max_iter):
    """STLSQ of one target (column `tcol` of G) on the Gram route, ``SINDy.train``'s loop.  Returns (coef [nf],
    bad, smallest squared pivot, smallest threshold margin, solves)."""
    keep = np.ones(nf, dtype=bool)
    coef = np.zeros(nf)
    bad, minp, margin, iters = False, np.inf, np.inf, 0
    for _ in range(max_iter):
        if not keep.any():
            break
        kl = np.nonzero(keep)[0]
        S = G[np.ix_(kl, kl)] + alpha * np.eye(len(kl))
        w, p = _scaled_cholesky_1(S, G[kl, tcol])
        if w is None or not np.all(np.isfinite(w)):
            return np.full(nf, np.nan), True, (p if w is None else min(minp, p)), margin, iters
        iters += 1
        minp = min(minp, p)
        if p < len(kl) * PIVOT_EPS:
            bad = True
        coef[:] = 0.0
        coef[kl] = w
        if threshold > 0:
            margin = min(margin, float(np.min(np.abs(np.abs(w) - threshold) / threshold)))
        small = np.abs(coef) < threshold
        if bad or not (small & keep).any():
            break
        keep &= ~small
    if bad:
        return np.full(nf, np.nan), True, minp, margin, iters
    return np.where(keep, coef, 0.0), False, minp, margin, iters


def stlsq_gram_host(traj_len, obs, ctrls, designs, configs, ycont=None, alpha=0.05, max_iter=20):
    """``_lib.sindy_fit`` in numpy: one Gram per design summed over 512-row blocks in order, sub-selection, scaled
    Cholesky, the same status rules.  Returns (coeffs, status, min_pivot, min_margin, iterations)."""
    if max_iter < 1:
        raise ValueError("max_iter < 1")
    lens = np.asarray(traj_len, dtype=np.int64)
    obs, ctrls = np.asarray(obs, dtype=np.float64), np.asarray(ctrls, dtype=np.float64)
    nx = obs.shape[1]
    if any(c[1] for c in configs) and ycont is None:
        raise ValueError("a continuous configuration needs continuous targets")
    used = {int(c[0]) for c in configs}
    grams = {d: design_gram(lens, obs, ctrls, designs[d], ycont) for d in used}
    coeffs, status, pivot, margin, iters = [], [], [], [], []
    for d, continuous, threshold in configs:
        G, nf = grams[int(d)], len(designs[int(d)][0])
        res = [stlsq_gram(G, nf, nf + (nx if continuous else 0) + j, float(threshold), alpha, max_iter)
               for j in range(nx)]
        bad = any(r[1] for r in res)
        m = min(r[3] for r in res)
        coeffs.append(np.array([r[0] for r in res]))
        status.append(1 if bad else 2 if m < TIE_MARGIN else 0)
        pivot.append(min(r[2] for r in res))
        margin.append(m)
        iters.append(max(r[4] for r in res))
    return (coeffs, np.array(status, dtype=np.int32), np.array(pivot), np.array(margin),
            np.array(iters, dtype=np.int32))


class SindyFitReport(list):
    """One entry per model, in order: ``{"where": "device" | "host", "reason": None | str, "route": None | "narrow" |
    "wide", "pivot", "margin", "iters"}`` (route: the Gram call that took the model, None when none did; the last
    three None then).  ``host_fits``: the ``train()`` calls that
    were made (equal configurations share one); ``device_fits``: configurations fitted on the Gram route;
    ``designs``: Grams formed."""
    host_fits = 0
    device_fits = 0
    designs = 0


def _library_key(m):
    return tuple((a.dtype.str, a.tobytes()) for a in m.library)


def _config_key(m):
    return (type(m), _library_key(m), m.time_mode, float(m.threshold))


def _host_reason(m, max_features=MAX_FEATURES):
    """Why a model cannot take the Gram route (None: it can)."""
    if type(m).train is not SINDy.train:
        return "subclass"
    if (len(m.library[0]) > max_features or m.system.obs_dim > MAX_STATE
            or not 1 <= m.system.ctrl_dim <= MAX_CTRL):
        return "size"
    return None


def continuous_targets(trajs, dt, xdot=None):
    """[R][nx]: per data row the derivative ``train()`` regresses on in continuous mode (the caller's `xdot`, or
    ``np.gradient`` of each trajectory's observations)."""
    if xdot is not None:
        return np.concatenate([np.asarray(d, dtype=np.float64) for d in xdot])
    return np.concatenate([np.gradient(t.obs, dt, axis=0) for t in trajs])


def fit_sindy_models(models, trajs, xdot=None, alpha=0.05, max_iter=20, device=0, backend="device", wide="host"):
    """Fit untrained ``SINDy`` models of one system to `trajs`; every model ends up as after its own
    ``train(trajs, xdot=xdot, alpha=alpha, max_iter=max_iter)``.  Equal configurations are fitted once, models with
    equal libraries share a design.  Models the Gram route declines (module docstring) are fitted by ``train()``.
    backend="numpy" runs ``stlsq_gram_host`` in place of the device call (the check of the algorithm on a host without
    a GPU; there is no automatic fallback).  wide="device": models whose library has 273..2048 features take the
    Gram route as well, in one ``ampc_sindy_fit_wide`` call next to the narrow one (backend="numpy":
    ``stlsq_gram_host``, which has no limit); "host": they are fitted by ``train()`` (reason "size").  Returns a
    ``SindyFitReport``."""
    if backend not in ("device", "numpy"):
        raise ValueError("backend must be 'device' or 'numpy'")
    if wide not in ("host", "device"):
        raise ValueError("wide must be 'host' or 'device'")
    max_features = MAX_FEATURES_WIDE if wide == "device" else MAX_FEATURES
    models = list(models)
    for m in models:
        if not isinstance(m, SINDy):
            raise TypeError("fit_sindy_models fits SINDy models, not %s" % type(m).__name__)
        if m.system != models[0].system:
            raise ValueError("fit_sindy_models: the models must share one system")
    report = SindyFitReport({"where": None, "reason": None, "route": None, "pivot": None, "margin": None,
                             "iters": None} for _ in models)
    groups = {}                                            # configuration -> indices of its models
    for i, m in enumerate(models):
        groups.setdefault(_config_key(m), []).append(i)
    short = xdot is None and any(len(t) < 2 for t in trajs)
    dev_keys, host = [], {}                                # host: configuration -> reason
    for key, members in groups.items():
        m = models[members[0]]
        reason = _host_reason(m, max_features)
        if reason is None and m.time_mode == "continuous" and short:
            reason = "short trajectory"                    # np.gradient raises in train(): let it
        if reason is None:
            dev_keys.append(key)
        else:
            host[key] = reason
    stats = {}
    if dev_keys:
        lens, obs, ctrls = concat_trajs(trajs)
        ycont = None
        if any(k[2] == "continuous" for k in dev_keys):
            ycont = continuous_targets(trajs, models[0].system.dt, xdot)
        narrow = [k for k in dev_keys if len(models[groups[k][0]].library[0]) <= MAX_FEATURES]
        routes = (("narrow", narrow, _lib.sindy_fit), ("wide", [k for k in dev_keys if k not in narrow],
                                                         _lib.sindy_fit_wide))
        for route, keys, call in routes:                   # one call per kernel family
            if not keys:
                continue
            design_of, designs = {}, []
            configs = []
            for key in keys:
                if key[1] not in design_of:
                    design_of[key[1]] = len(designs)
                    designs.append(models[groups[key][0]].library)
                configs.append((design_of[key[1]], key[2] == "continuous", key[3]))
            report.designs += len(designs)
            if backend == "device":
                out = call(lens, obs, ctrls, designs, configs, ycont=ycont, alpha=alpha, max_iter=max_iter,
                           device=device)
            else:
                out = stlsq_gram_host(lens, obs, ctrls, designs, configs, ycont=ycont, alpha=alpha, max_iter=max_iter)
            for key, c, s, p, mg, it in zip(keys, *out):
                stats[key] = {"route": route, "pivot": float(p), "margin": float(mg), "iters": int(it)}
                if s != 0:
                    host[key] = "status %d" % s
                    continue
                for i in groups[key]:
                    models[i].set_coefficients(c)
                    report[i].update(where="device", **stats[key])
                report.device_fits += 1
    for key, reason in host.items():
        first = models[groups[key][0]]
        first.train(trajs, xdot=xdot, silent=True, alpha=alpha, max_iter=max_iter)
        report.host_fits += 1
        for i in groups[key]:
            if models[i] is not first:
                models[i].set_coefficients(first.coefficients)
            report[i].update(where="host", reason=reason, **stats.get(key, {}))
    return report
