"""Batched least-squares fits of ARX and Koopman(lstsq) models: one Gram pass, one small solve per model.

``ARX.train`` (reference arx.py:78-116) builds the ``[rows, 1 + k (no + nu)]`` design matrix and runs one SVD
least-squares solve per observation column; ``Koopman.train`` (koopman.py:141-154) a pseudo-inverse of the lifted
data.  A tuner asks for many such fits of ONE data set.  The feature vector of ARX history ``k`` is a prefix of the
feature vector of the longest history plus its two trailing blocks (constant, current control), so one Gram matrix
``F'[F | Y]`` of the widest design holds the normal equations of every history as a sub-matrix; Koopman
configurations of one basis share a Gram.  ``fit_linear_models`` forms the Grams on the device (``ampc_linfit_fit``:
design rows built on the fly, f64 MFMA, fixed-order sums) and solves every configuration there by a Cholesky
factorisation of the unit-diagonal Gram.

When the device declines.  The scaled Gram has unit diagonal, so a squared pivot is ``1 - R^2`` of that column
against the ones before it.  A configuration whose smallest squared pivot is below ``n_features * 2^-26`` (or not
positive) comes back with status 1 -- the normal equations squared its condition number past half the digits -- and
its model is fitted by its own ``train()``.  So are models the Gram route cannot express or whose reference result
is not a stable target: Koopman with ``method`` other than ``"lstsq"``, with product terms, with DUPLICATE basis
functions (``strict_reference=True`` reproduces the reference's late-binding lambdas, so ``poly_degree >= 3`` or a
trig basis with ``poly_degree >= 2`` yields identical columns; the reference's answer is then whatever its
pseudo-inverse cutoff makes of singular values at rounding level), and models over the device limits (256 states,
16 controls).  Every model ends up exactly as after its own ``train(trajs)``: ARX through ``_set_coeffs``, Koopman
through ``_set_matrices``.

Lasso.  With ``lasso="device"`` Koopman models of ``method="lasso"`` take a Gram route of their own
(``sysid/lasso_fit.py``, ``ampc_lasso_fit``: sklearn's cyclic coordinate descent run on the centred Gram of
``[1 | F | Y]``, one Gram per distinct basis whatever the alphas).  Duplicate basis functions are allowed there
(coordinate descent is well defined on them); product terms and over-size models still go to ``train()``, and so do
configurations that come back with status 1 (centring lost half the digits of a column, or a non-finite value) or
status 2 (a stopping decision too close to call).  The default ``lasso="host"`` leaves every lasso model to
``train()``, as before.

Stable.  With ``stable="device"`` Koopman models of ``method="stable"`` take the Gram route of
``sysid/stable_fit.py`` (``ampc_stable_fit``: the reference's projected fast-gradient method run on the Gram of
``[F | Y]``, one configuration per distinct basis).  Models with product terms are refused as by ``train()``; models
over that route's limits (64 lifted states, 16 controls) and configurations that come back with status 1 (a Cholesky
pivot under the rule above -- duplicate basis functions end here --, an ill-conditioned polar factor, a non-finite
value) or status 2 (a line-search decision too close to call) are fitted by ``stable_fit.stabilize_host``, the
reference's routine restated on the data.  The default ``stable="host"`` leaves every stable model to ``train()``,
which refuses the method, as before.

``gram_fit_host`` is the same algorithm in numpy (what the CPU tests run and the GPU tests compare against first).
"""
import numpy as np

from .. import _lib
from .linear import ARX, Koopman

MAX_STATE, MAX_CTRL, MAX_POWER = 256, 16, 64
SPLIT_ROWS = 512                       # rows per partial sum (the device's kLinfitSplitRows)
PIVOT_EPS = 2.0 ** -26                 # ~ sqrt(eps): acceptance threshold per feature


def concat_trajs(trajs):
    """(traj_len, obs [R][no], ctrls [R][nu]): the trajectories concatenated, as ampc_kstep_errors takes them."""
    lens = np.array([len(t) for t in trajs], dtype=np.int32)
    obs = np.concatenate([np.asarray(t.obs, dtype=np.float64) for t in trajs])
    ctrls = np.concatenate([np.asarray(t.ctrls, dtype=np.float64) for t in trajs])
    return lens, np.ascontiguousarray(obs), np.ascontiguousarray(ctrls)


def _row_start(lens):
    """Per concatenated row: the first row of its trajectory, and whether it has a successor."""
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    start = np.repeat(starts, lens)
    t = np.arange(int(np.sum(lens))) - start
    return start, t + 1 < np.repeat(lens, lens)


def arx_design(lens, obs, ctrls, history):
    """(F, Y) of ARX history `history`: rows in data order, columns in ARX's own feature order
    (ARX._get_all_feature_vectors), the lag gather clamped to the row's own trajectory."""
    no, nu, k = obs.shape[1], ctrls.shape[1], int(history)
    start, valid = _row_start(lens)
    g = np.nonzero(valid)[0]
    F = np.zeros((len(g), 1 + k * (no + nu)))
    F[:, :no] = obs[g]
    j = no
    for i in range(1, k):
        idx = np.maximum(g - i, start[g])
        F[:, j:j + no] = obs[idx]
        j += no
        F[:, j:j + nu] = ctrls[idx]
        j += nu
    F[:, -(nu + 1)] = 1.0
    F[:, -nu:] = ctrls[g]
    return F, obs[g + 1]


def lift(obs, basis):
    """Basis functions (kinds, params) applied element-wise, basis-major (Koopman._apply_basis)."""
    parts = []
    for kind, p in zip(*basis):
        kind = int(kind)
        parts.append(obs if kind == 0 else obs ** int(p) if kind == 1
                     else np.sin(p * obs) if kind == 2 else np.cos(p * obs))
    return np.concatenate(parts, axis=-1)


def koopman_design(lens, obs, ctrls, basis):
    """(F, Y) of a Koopman basis: F = [lift(obs[t]), ctrls[t]], Y = lift(obs[t + 1])."""
    _, valid = _row_start(lens)
    g = np.nonzero(valid)[0]
    Z = lift(obs, basis)
    return np.concatenate([Z[g], ctrls[g]], axis=1), Z[g + 1]


def host_gram(F, Y, ordered=False):
    """G = F'[F | Y], summed over blocks of SPLIT_ROWS rows in order.  ordered=True adds the rows one at a
    time instead: an entry is then the same bits whatever other columns the design holds."""
    FY = np.concatenate([F, Y], axis=1)
    G = np.zeros((F.shape[1], FY.shape[1]))
    if ordered:
        for r in range(F.shape[0]):
            G += np.multiply.outer(F[r], FY[r])
        return G
    for r0 in range(0, F.shape[0], SPLIT_ROWS):
        G += F[r0:r0 + SPLIT_ROWS].T @ FY[r0:r0 + SPLIT_ROWS]
    return G


def arx_columns(history, kmax, no, nu):
    """Columns of the history-`kmax` design that make up history `history`'s: the prefix and the two trailing
    blocks (constant, current control)."""
    nf = 1 + kmax * (no + nu)
    return np.concatenate([np.arange(no + (history - 1) * (no + nu)), np.arange(nf - nu - 1, nf)])


def solve_scaled_cholesky(G, idx, tcol, nt):
    """Coefficients [nt][n] of the sub-problem `idx` of G (targets: columns tcol .. tcol + nt), status and the
    smallest squared pivot: D G D with D = diag(G)^-1/2 factored by a right-looking Cholesky, the right-hand sides
    carried as extra rows; status 1 when a pivot is not positive and finite or the smallest is below n * 2^-26."""
    idx = np.asarray(idx)
    n = len(idx)
    diag = G[idx, idx]
    nan = np.full((nt, n), np.nan)
    if not (np.all(diag > 0) and np.all(np.isfinite(diag))):
        return nan, 1, float(np.min(diag))
    d = 1.0 / np.sqrt(diag)
    M = np.empty((n + nt, n))
    M[:n] = G[np.ix_(idx, idx)] * d[:, None] * d[None, :]
    M[n:] = (G[idx, tcol:tcol + nt] * d[:, None]).T
    minp = np.inf
    for j in range(n):
        p = M[j, j]
        if not (p > 0 and np.isfinite(p)):
            return nan, 1, float(p)
        minp = min(minp, p)
        M[j, j] = np.sqrt(p)
        M[j + 1:, j] /= M[j, j]
        M[j + 1:, j + 1:] -= np.multiply.outer(M[j + 1:, j], M[j + 1:n, j])
    y = M[n:]
    for j in range(n - 1, -1, -1):
        y[:, j] /= M[j, j]
        y[:, :j] -= np.multiply.outer(y[:, j], M[j, :j])
    coef = y * d[None, :]
    if not np.all(np.isfinite(coef)):
        return nan, 1, float(minp)
    return coef, int(minp < n * PIVOT_EPS), float(minp)


def gram_fit_host(traj_len, obs, ctrls, arx_histories=(), koopman_bases=(), ordered=False):
    """``_lib.linfit_fit`` in numpy: one Gram of the longest ARX history and one per distinct Koopman basis,
    sub-selection, scaled Cholesky, the same acceptance rule.  Returns (coeffs, status, min_pivot), ARX first."""
    lens = np.asarray(traj_len, dtype=np.int64)
    obs, ctrls = np.asarray(obs, dtype=np.float64), np.asarray(ctrls, dtype=np.float64)
    no, nu = obs.shape[1], ctrls.shape[1]
    out = []
    if len(arx_histories):
        kmax = int(max(arx_histories))
        F, Y = arx_design(lens, obs, ctrls, kmax)
        G = host_gram(F, Y, ordered)
        for k in arx_histories:
            out.append(solve_scaled_cholesky(G, arx_columns(int(k), kmax, no, nu), F.shape[1], no))
    grams = {}
    for kinds, params in koopman_bases:
        key = (tuple(int(k) for k in kinds), tuple(float(p) for p in params))
        if key not in grams:
            F, Y = koopman_design(lens, obs, ctrls, key)
            grams[key] = (host_gram(F, Y, ordered), F.shape[1], Y.shape[1])
        G, nf, nt = grams[key]
        out.append(solve_scaled_cholesky(G, np.arange(nf), nf, nt))
    return ([o[0] for o in out], np.array([o[1] for o in out], dtype=np.int32),
            np.array([o[2] for o in out], dtype=np.float64))


class LinearFitReport(list):
    """One entry per model, in order: ``{"where": "device" | "host", "reason": None | str, "pivot": float |
    None}``; models that took the lasso route also carry ``"sweeps"`` and ``"margin"``, models of the stable route
    ``"iterations"``, ``"trials"``, ``"margin"`` and ``"error"``.  ``host_fits``: the ``train()`` calls that were made (equal configurations share one)."""
    host_fits = 0
    device_fits = 0


def _config_key(m):
    if isinstance(m, ARX):
        return ("arx", m.k)
    return ("koopman", m.method, m.lasso_alpha, tuple(m.basis), m.product_terms)


def _host_reason(m, lasso="host", stable="host"):
    """Why a model cannot take a Gram route (None: it can)."""
    no, nu = m.system.obs_dim, m.system.ctrl_dim
    if nu > MAX_CTRL or no > MAX_STATE:
        return "size"
    if isinstance(m, ARX):
        return "size" if m.state_dim > MAX_STATE else None
    if stable == "device" and m.method == "stable":
        from .stable_fit import MAX_N                      # here, not at the top: stable_fit imports this module
        if m.product_terms:
            return "product_terms"
        if len(m.basis) * no > MAX_N or any(k == 1 and not 0 <= p <= MAX_POWER for k, p in m.basis):
            return "size"
        return None
    on_lasso_route = lasso == "device" and m.method == "lasso" and m.lasso_alpha is not None
    if m.method != "lstsq" and not on_lasso_route:
        return "method"
    if m.product_terms:
        return "product_terms"
    if len(set(m.basis)) != len(m.basis) and not on_lasso_route:
        return "duplicate basis"
    if len(m.basis) * no > MAX_STATE or any(k == 1 and not 0 <= p <= MAX_POWER for k, p in m.basis):
        return "size"
    return None


def _copy_fit(src, dst):
    if isinstance(src, ARX):
        dst._set_coeffs(src.coeffs)
    else:
        dst._set_matrices(src.A, src.B)


def _stable_host_fit(m, trajs):
    """A stable Koopman model fitted by the data-form restatement of the reference's routine."""
    from .stable_fit import koopman_rows, stabilize_host
    lens, obs, ctrls = concat_trajs(trajs)
    stats = {}
    A, B, error = stabilize_host(*koopman_rows(lens, obs, ctrls, m.device_lift()), stats=stats)
    m._set_matrices(A, B)
    return dict(stats, error=error)


def fit_linear_models(models, trajs, device=0, backend="device", lasso="host", stable="host"):
    """Fit untrained ``ARX`` / ``Koopman`` models of one system to `trajs`; every model ends up as after its own
    ``train(trajs)``.  Equal configurations are fitted once.  Models the Gram route declines (module docstring)
    are fitted by ``train()``.  backend="numpy" runs ``gram_fit_host`` in place of the device call (the check of
    the algorithm on a host without a GPU; there is no automatic fallback).  lasso="device": Koopman models of
    method "lasso" are fitted by ``ampc_lasso_fit`` (backend="numpy": ``lasso_fit_host``), their report entries gain
    ``"sweeps"`` and ``"margin"``; lasso="host" (default): by ``train()``.  stable="device": Koopman models of method
    "stable" (without product terms) are fitted by ``ampc_stable_fit`` (backend="numpy": ``stable_fit_host``), those it
    declines by ``stabilize_host``; their report entries gain ``"iterations"``, ``"trials"``, ``"margin"`` and
    ``"error"``; stable="host" (default): by ``train()``, which refuses the method.  Returns a ``LinearFitReport``."""
    if backend not in ("device", "numpy"):
        raise ValueError("backend must be 'device' or 'numpy'")
    if lasso not in ("host", "device"):
        raise ValueError("lasso must be 'host' or 'device'")
    if stable not in ("host", "device"):
        raise ValueError("stable must be 'host' or 'device'")
    models = list(models)
    for m in models:
        if not isinstance(m, (ARX, Koopman)):
            raise TypeError("fit_linear_models fits ARX and Koopman models, not %s" % type(m).__name__)
        if m.system != models[0].system:
            raise ValueError("fit_linear_models: the models must share one system")
    report = LinearFitReport({"where": None, "reason": None, "pivot": None} for _ in models)
    groups = {}                                            # configuration -> indices of its models
    for i, m in enumerate(models):
        groups.setdefault(_config_key(m), []).append(i)
    dev_keys, lasso_keys, stable_keys, host = [], [], [], {}       # host: configuration -> reason
    stable_host = {}                                       # stable configurations for stabilize_host -> reason
    for key, members in groups.items():
        reason = _host_reason(models[members[0]], lasso, stable)
        on_stable_route = stable == "device" and key[0] == "koopman" and key[1] == "stable"
        if on_stable_route and reason == "size":
            stable_host[key] = reason
        elif reason is not None:
            host[key] = reason
        elif on_stable_route:
            stable_keys.append(key)
        elif key[0] == "koopman" and key[1] == "lasso":
            lasso_keys.append(key)
        else:
            dev_keys.append(key)
    pivots = {}
    if lasso_keys:
        from .lasso_fit import lasso_fit_host
        lens, obs, ctrls = concat_trajs(trajs)
        basis_of, bases, configs = {}, [], []
        for key in lasso_keys:
            if key[3] not in basis_of:
                basis_of[key[3]] = len(bases)
                bases.append(models[groups[key][0]].device_lift())
            configs.append((basis_of[key[3]], float(key[2])))
        if backend == "device":
            out = _lib.lasso_fit(lens, obs, ctrls, bases, configs, device=device)
        else:
            out = lasso_fit_host(lens, obs, ctrls, bases, configs)
        for key, c, s, mg, sw in zip(lasso_keys, *out):
            stats = {"sweeps": int(sw), "margin": float(np.min(mg))}
            for i in groups[key]:
                report[i].update(stats)
            if s != 0:
                host[key] = "status %d" % s
                continue
            n = c.shape[0]
            for i in groups[key]:
                models[i]._set_matrices(c[:n, :n], c[:n, n:])
                report[i].update(where="device")
            report.device_fits += 1
    if stable_keys:
        from .stable_fit import stable_fit_host
        lens, obs, ctrls = concat_trajs(trajs)
        bases = [models[groups[key][0]].device_lift() for key in stable_keys]
        if backend == "device":
            out = _lib.stable_fit(lens, obs, ctrls, bases, device=device)
        else:
            out = stable_fit_host(lens, obs, ctrls, bases)
        for key, c, s, err, it, tr, mg in zip(stable_keys, *out):
            if s != 0:
                stable_host[key] = "status %d" % s
                continue
            stats = {"iterations": int(it), "trials": int(tr), "margin": float(mg), "error": float(err)}
            n = c.shape[0]
            for i in groups[key]:
                models[i]._set_matrices(c[:n, :n], c[:n, n:])
                report[i].update(stats, where="device")
            report.device_fits += 1
    for key, reason in stable_host.items():
        first = models[groups[key][0]]
        stats = _stable_host_fit(first, trajs)
        report.host_fits += 1
        for i in groups[key]:
            if models[i] is not first:
                _copy_fit(first, models[i])
            report[i].update(stats, where="host", reason=reason)
    if dev_keys:
        lens, obs, ctrls = concat_trajs(trajs)
        arx = [k for k in dev_keys if k[0] == "arx"]
        koop = [k for k in dev_keys if k[0] == "koopman"]
        bases = [models[groups[k][0]].device_lift() for k in koop]
        fit = _lib.linfit_fit if backend == "device" else gram_fit_host
        kw = {"device": device} if backend == "device" else {}
        coeffs, status, pivot = fit(lens, obs, ctrls, [k[1] for k in arx], bases, **kw)
        for key, c, s, p in zip(arx + koop, coeffs, status, pivot):
            pivots[key] = float(p)
            if s != 0:
                host[key] = "status 1"
                continue
            for i in groups[key]:
                m = models[i]
                if isinstance(m, ARX):
                    m._set_coeffs(c)
                else:
                    n = c.shape[0]
                    m._set_matrices(c[:n, :n], c[:n, n:])
                report[i].update(where="device", pivot=pivots[key])
            report.device_fits += 1
    for key, reason in host.items():
        first = models[groups[key][0]]
        first.train(trajs, silent=True)
        report.host_fits += 1
        for i in groups[key]:
            if models[i] is not first:
                _copy_fit(first, models[i])
            report[i].update(where="host", reason=reason, pivot=pivots.get(key))
    return report
