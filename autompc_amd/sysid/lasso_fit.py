"""Lasso fits of Koopman models on the Gram route: cyclic coordinate descent on one centred Gram per basis.

``Koopman.train`` with ``method="lasso"`` runs ``sklearn.linear_model.Lasso(alpha).fit(XU.T, Y.T)`` (koopman.py:150-156):
per lifted target a residual-form cyclic coordinate descent, every sweep touching all design rows, with sklearn's
defaults (``fit_intercept=True``, ``max_iter=1000``, ``tol=1e-4``, cyclic selection, not positive; the intercept is
dropped).  Everything that descent needs is in the Gram of the design ``[1 | F | Y]``, ``F = [lift(obs[t]), ctrls[t]]``,
``Y = lift(obs[t + 1])``.  With m rows, ``mu = sum F / m`` and ``ybar = sum Y / m`` (the constant column supplies the
sums):

    G = F'F - m mu mu'        Q = F'Y - m mu ybar'        yy_t = Y_t'Y_t - m ybar_t^2
    alpha = lasso_alpha m     tol_t = 1e-4 yy_t

Per target t, from ``w = 0`` and ``H = G w = 0``, sweeps ``it = 0 .. 999`` over the features in order:

    skip i if G_ii == 0
    tmp = Q_it - H_i + w_i G_ii ;  w_new = sign(tmp) max(|tmp| - alpha, 0) / G_ii
    if w_new != w_i:  H += (w_new - w_i) G[:, i]
    d_w_max = max |w_new - w_i| ;  w_max = max |w_new|

and after the sweep, when ``w_max == 0`` or ``d_w_max / w_max < 1e-4`` or ``it == 999``, the duality gap

    dn = max |Q_t - H| ;  R2 = yy_t - 2 w.Q_t + w.H ;  Ry = yy_t - w.Q_t
    dn > alpha:  c = alpha / dn, gap = (R2 + R2 c^2) / 2      else  c = 1, gap = R2
    gap += alpha |w|_1 - c Ry ;  stop when gap < tol_t

A sweep costs n_features^2 flops instead of rows x n_features, the targets are independent.  A sweep that changes no
coefficient and does not stop would repeat unchanged to the cap, so its count is set to the cap at once.  A target
that reaches sweep 1000 keeps its ``w`` (sklearn warns and does the same).

Status per configuration.  0: fitted (targets that ran the cap included).  1, not fitted here: a quantity is not
finite, or the centring took half the digits of some column's sum of squares -- ``G_ii < 2^-26 (F'F)_ii`` for a
feature, ``yy_t < 2^-26 Y_t'Y_t`` for a target, raw value non-zero (``PIVOT_EPS``'s half-precision rule; a column
that is exactly zero is no reason: it is skipped and keeps coefficient 0).  2, a decision too close to call: at some
gap check ``|gap - tol_t| <= TIE tol_t``, or at some sweep ``|d_w_max / w_max - 1e-4| <= RATIO_TIE 1e-4``; the smallest
margin of either kind is returned.  The Gram-form gap differs from sklearn's residual-form gap by rounding, and the
device's Gram sums from numpy's in the last bits: a decision that close could go the other way there, and the fits
would then differ by whole sweeps.  Models with status 1 or 2 are fitted by their own ``train()``.

The two margins.  ``TIE`` is 100 x the largest ``|gap_Gram - gap_residual| / tol_t`` measured over every gap check of
the test cases (2.4e-5, in the duplicate basis at alpha 1e-5: there ``dn`` is a difference of two numbers 1e5 times
its size and ``c = alpha / dn`` carries 1e-8).  One case does not enter: ``near``, whose jittered control keeps 4.1e-8 of
its sum of squares, 2.7 x the ``2^-26`` line of status 1.  Its gap form departs by 1.3e-4 and its coefficients by
3.7e-8, both the conditioning of that one column; 1.3e-4 is still 18 times inside ``TIE`` (held by a test), while a
``TIE`` of 100 x 1.3e-4 would call a tie in nearly every design of 192 features or more (no seed in 600 of the sweep
cases of 192, 256 and 257 features stays clear of 1.4e-2), and a ``RATIO_TIE`` from 3.7e-8 in every fit.  That figure
says nothing about the sweep test, which reads only ``w``:
the restatement's coefficients differ from sklearn's by at most 4e-12 of max|w| on those cases, a difference of two
of them at the decision (``d_w_max = 1e-4 w_max``) therefore by 4e-8 of itself, and ``RATIO_TIE`` is 100 x that.  One
constant for both would either not cover the gap (4e-6) or call a tie in most fits of a few hundred sweeps (2.4e-3:
with thousands of (target, sweep) decisions the closest ratio lies about 1e-4 .. 1e-5 from 1e-4).

``lasso_fit_host`` is the algorithm in numpy (what the CPU tests run and the GPU tests compare against);
``_lib.lasso_fit`` (``ampc_lasso_fit``) runs it on the device.
"""
import numpy as np

from .linear_fit import PIVOT_EPS, SPLIT_ROWS, _row_start, lift

MAX_ITER, TOL = 1000, 1e-4             # sklearn's Lasso defaults
# Largest |gap_Gram - gap_residual| / tol_t over every gap check of the cases of tests/lassofit_cases.py, sklearn's
# residual-form gap evaluated in numpy at the same w (tests/golden/gen_golden_lassofit.py prints it; the case near,
# a column 2.7 x 2^-26 from status 1, is listed apart: see the module docstring) ...
GAP_FORM_ERROR = 2.4e-5
TIE = 100.0 * GAP_FORM_ERROR           # ... and the margin below which a gap decision counts as a tie
# Largest max|coef - sklearn's| / max|coef| of the restatement on those cases (near apart), as a fraction of the 1e-4
# the sweep test compares d_w_max / w_max with, and the margin below which that decision counts as a tie
RATIO_FORM_ERROR = 4.0e-12 / TOL
RATIO_TIE = 100.0 * RATIO_FORM_ERROR


def centred_gram(lens, obs, ctrls, basis):
    """(G [nf][nf], Q [nf][nt], yy [nt], raw diagonal of F'F [nf], raw Y_t'Y_t [nt], m) of one basis: the Gram of
    [1 | F | Y] summed over blocks of SPLIT_ROWS data rows in order (the device's row splits), centred through its
    constant column."""
    _, valid = _row_start(lens)
    Z = lift(obs, basis)
    nt, nf = Z.shape[1], Z.shape[1] + ctrls.shape[1]
    raw = np.zeros((1 + nf, 1 + nf + nt))
    yraw = np.zeros(nt)
    m = 0
    for r0 in range(0, obs.shape[0], SPLIT_ROWS):
        g = r0 + np.nonzero(valid[r0:r0 + SPLIT_ROWS])[0]
        if not len(g):
            continue
        D = np.concatenate([np.ones((len(g), 1)), Z[g], ctrls[g], Z[g + 1]], axis=1)
        raw += D[:, :1 + nf].T @ D
        yraw += np.sum(D[:, 1 + nf:] * D[:, 1 + nf:], axis=0)
        m += len(g)
    mu, ybar = raw[0, 1:1 + nf] / m, raw[0, 1 + nf:] / m
    FF = raw[1:, 1:1 + nf]
    FF = np.triu(FF) + np.triu(FF, 1).T                     # one summation per pair: exactly symmetric
    G = FF - m * np.multiply.outer(mu, mu)
    Q = raw[1:, 1 + nf:] - m * np.multiply.outer(mu, ybar)
    yy = yraw - m * (ybar * ybar)
    return G, Q, yy, np.diagonal(FF).copy(), yraw, m


def coordinate_descent(G, Q, yy, alpha, max_iter=MAX_ITER, tol=TOL, gap_log=None):
    """The sweeps of the module docstring for all targets of one (Gram, alpha); the targets run side by side, each
    element-wise exactly as on its own.  Returns (W [nt][nf], sweeps [nt], margin [nt][2]: the smallest gap margin
    and the smallest sweep-test margin); gap_log, a list, receives (target, w, gap, tol_t) of every gap check."""
    nf, nt = Q.shape
    W, H = np.zeros((nt, nf)), np.zeros((nt, nf))
    sweeps = np.zeros(nt, dtype=np.int32)
    margin = np.full((nt, 2), np.inf)
    tols = tol * yy
    diag = np.diagonal(G)
    live = [i for i in range(nf) if diag[i] != 0]
    active = np.arange(nt)
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            if not len(active):
                break
            a = active
            w, h, q = W[a], H[a], Q[:, a].T
            dmax, wmax = np.zeros(len(a)), np.zeros(len(a))
            for i in live:
                wi = w[:, i].copy()
                tmp = q[:, i] - h[:, i] + wi * diag[i]
                wn = np.sign(tmp) * np.maximum(np.abs(tmp) - alpha, 0.0) / diag[i]
                ch = wn != wi
                if ch.any():
                    h[ch] += (wn[ch] - wi[ch])[:, None] * G[i][None, :]
                w[:, i] = wn
                dmax, wmax = np.maximum(dmax, np.abs(wn - wi)), np.maximum(wmax, np.abs(wn))
            W[a], H[a] = w, h
            sweeps[a] = it + 1
            ratio = np.where(wmax > 0, dmax / np.where(wmax > 0, wmax, 1.0), 0.0)
            margin[a, 1] = np.minimum(margin[a, 1], np.where(wmax > 0, np.abs(ratio - tol) / tol, np.inf))
            check = (wmax == 0) | (ratio < tol) | (it == max_iter - 1)
            stop = np.zeros(len(a), dtype=bool)
            for k in np.nonzero(check)[0]:
                t = a[k]
                dn = np.max(np.abs(q[k] - h[k])) if nf else 0.0
                wq, wh = float(w[k] @ q[k]), float(w[k] @ h[k])
                r2, ry = yy[t] - 2.0 * wq + wh, yy[t] - wq
                if dn > alpha:
                    c = alpha / dn
                    gap = 0.5 * (r2 + r2 * (c * c))
                else:
                    c, gap = 1.0, r2
                gap += alpha * float(np.sum(np.abs(w[k]))) - c * ry
                if tols[t] > 0:
                    margin[t, 0] = min(margin[t, 0], abs(gap - tols[t]) / tols[t])
                if gap_log is not None:
                    gap_log.append((int(t), w[k].copy(), float(gap), float(tols[t])))
                stop[k] = gap < tols[t]
            frozen = (dmax == 0) & ~stop                   # nothing moved: every later sweep is this one again
            sweeps[a[frozen]] = max_iter
            active = a[~(stop | frozen)]
    return W, sweeps, margin


def lasso_fit_host(traj_len, obs, ctrls, bases, configs, tie=TIE, ratio_tie=RATIO_TIE, per_target=False,
                   gap_log=None):
    """``_lib.lasso_fit`` in numpy.  bases: (kinds, params) pairs; configs: (basis index, lasso_alpha) pairs.
    Returns (coeffs, status, min_margin, sweeps): a list of [n][n + nu] matrices and three per-configuration arrays
    (min_margin [.][2]: gap and sweep-test margin; sweeps: the largest over the targets); per_target=True appends the list of per-target sweep counts.  gap_log:
    a list that receives (configuration, target, w, gap, tol_t) of every gap check."""
    lens = np.asarray(traj_len, dtype=np.int64)
    obs, ctrls = np.asarray(obs, dtype=np.float64), np.asarray(ctrls, dtype=np.float64)
    grams = {}
    coeffs, status, margins, sweeps, detail = [], [], [], [], []
    for ci, (b, lasso_alpha) in enumerate(configs):
        b = int(b)
        if b not in grams:
            kinds, params = bases[b]
            key = (tuple(int(k) for k in kinds), tuple(float(p) for p in params))
            grams[b] = centred_gram(lens, obs, ctrls, key)
        G, Q, yy, fraw, yraw, m = grams[b]
        finite = all(np.all(np.isfinite(x)) for x in (G, Q, yy)) and np.isfinite(lasso_alpha)
        lost = bool(np.any((fraw != 0) & (np.diagonal(G) < PIVOT_EPS * fraw))
                    or np.any((yraw != 0) & (yy < PIVOT_EPS * yraw)))
        if not finite or lost:
            nt, nf = Q.shape[1], Q.shape[0]
            coeffs.append(np.full((nt, nf), np.nan))
            status.append(1)
            margins.append([np.inf, np.inf])
            sweeps.append(0)
            detail.append(np.zeros(nt, dtype=np.int32))
            continue
        log = None if gap_log is None else []
        W, its, mg = coordinate_descent(G, Q, yy, float(lasso_alpha) * m, gap_log=log)
        if gap_log is not None:
            gap_log.extend((ci,) + e for e in log)
        mmin = np.min(mg, axis=0)
        coeffs.append(W)
        status.append(1 if not np.all(np.isfinite(W)) else 2 if mmin[0] <= tie or mmin[1] <= ratio_tie else 0)
        margins.append(mmin)
        sweeps.append(int(np.max(its)) if len(its) else 0)
        detail.append(its)
    out = (coeffs, np.array(status, dtype=np.int32), np.array(margins, dtype=np.float64).reshape(-1, 2),
           np.array(sweeps, dtype=np.int32))
    return out + (detail,) if per_target else out
