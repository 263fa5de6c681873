"""Stable fits of Koopman models: a projected fast-gradient method on ``(S, U, B, Bcon)`` with ``A = S^-1 U B S``.

``Koopman`` with ``method="stable"`` is fitted in the reference by ``stabilize_discrete`` (stable_koopman.py:47-167):
``S`` positive definite, ``U`` orthogonal, ``B`` symmetric with eigenvalues in [0, 1], so that ``A = S^-1 U B S`` is
Schur stable by construction; the four factors are moved by a fast-gradient method (FGM weights, restart when the
line search fails), each line-search trial projecting ``S`` (eigenvalues clipped below at 1e-15), ``U`` (polar
factor) and ``B`` (eigenvalues clipped to [0, 1]) back and evaluating ``e = |Y - Bcon Xu - A Xs|_F`` over all design
rows.  At most 29 outer iterations, 20 trials each (100 in the first).

``stabilize_host`` restates that routine on the data (``eigh`` for the projections, the SVD for the polar factor):
the yardstick the goldens pin, and the fit of every model the Gram route declines.

The Gram form (``stable_fit_host``; ``ampc_stable_fit`` runs the same recursion on the device).  With ``F = [Xs; Xu]``
(features by rows), ``G = F F'``, ``Q = Y F'`` and the least-squares solution ``W0 = Q G^-1`` (the reference's
initialisation ``Y pinv(X)``; the scaled Cholesky of ``linear_fit.solve_scaled_cholesky``), the residual of ``W0`` is
orthogonal to ``F``, so for any ``W = [A | Bcon]``, ``D = W - W0``, ``T = D G``:

    e^2 = e0^2 + tr(T D')        e0^2 = |Y - W0 F|^2 = sum_t Y_t'Y_t - sum (W0 o Q)   (the Schur complement)
    -Error Xs' = T[:, :n]        -Error Xu' = T[:, n:]

and the four gradients follow from ``T``, ``S``, ``S^-1``, ``U`` and ``B``:

    t1 = S^-1 T[:, :n]     x1 = t1 S     x2 = U' t1
    gS = B x2 - t1 A'      gU = x1 B     gB = U' x1      gBcon = T[:, n:]

A trial costs O(n^3) whatever the number of rows.  The polar factor of ``M`` is ``M (M'M)^-1/2`` through the same
symmetric eigensolver as the two projections, followed by two Newton-Schulz steps ``U <- U (3 I - U'U) / 2`` (``M`` stays
near orthogonal except in the first, over-long trials of a line search; at the start ``M`` is the least-squares
``A``, and ``B = clip((M'M)^1/2)``); ``S^-1`` comes from the decomposition of ``S`` just computed, and so does the
ratio of its extreme eigenvalues that sets the step length after a restart.  The device decomposes by cyclic Jacobi in
the fixed parallel order of ``jacobi_eigh`` (``eig="jacobi"`` runs that here); ``eig="lapack"``, the default, uses
``numpy.linalg.eigh``.  The two are equally valid decompositions: the fits differ by rounding amplified through the
iteration, which is what the goldens' ``roundoff_response`` measures.

Status per basis.  0: fitted.  1, not fitted here: a Cholesky pivot under the rule of ``linear_fit`` (the basis has
(nearly) dependent functions), ``M'M`` of a polar factor with ``min eig <= 2^-40 max eig`` (``M (M'M)^-1/2`` then
departs from orthogonality by more than 1e-4, which the two Newton-Schulz steps that follow no longer take to rounding), an
eigen-iteration that did not converge within ``JACOBI_SWEEPS`` sweeps, or a value that is not finite.  2, a decision
too close to call: at some line-search trial ``|e_next - e| <= tie e``, or ``|e - 1e-12 |Y|_F| <= tie 1e-12 |Y|_F`` at
the convergence test -- the Gram-form error differs from the data-form error by rounding, and a decision that close
could go the other way there, after which the fits differ by whole trials.  Models with status 1 or 2 are fitted by
``stabilize_host``.
"""
import math

import numpy as np

from .linear_fit import PIVOT_EPS, SPLIT_ROWS, _row_start, lift, solve_scaled_cholesky

MAX_N, MAX_CTRL = 64, 16                 # lifted states and controls of the device route
MAX_OUTER, LS_MAX, LS_MAX_FIRST, LS_PARAM, ALPHA0 = 30, 20, 100, 1.5, 0.5      # stable_koopman.py:65-90
S_FLOOR, CONVERGED = 1e-15, 1e-12
POLAR_EPS = 2.0 ** -40                   # M'M of a polar factor must have min eig > POLAR_EPS max eig
JACOBI_SWEEPS = 30                       # sweep cap of the device's eigensolver
JACOBI_EPS = 2.0 ** -53                  # a pair is rotated when |a_pq| > JACOBI_EPS (|a_pp| + |a_qq|)
# Largest |e_Gram - e_data| / e_data at the same iterate over every error evaluation of every case of
# tests/stablefit_cases.py whose error is at most 10 x the error it is compared with (tests/golden/
# gen_golden_stablefit.py prints it, says why the over-long first trials of a line search are left out, and asserts
# that there both forms' errors are beyond 10 x the current one, so that no decision can turn).  3.5e-14 over the
# first six cases; the size sweep reaches 8.0e-13 (n = 2, 16 controls) and its ragged-rows case, whose long trajectory
# grows to |x| = 400 so that e0^2 is the difference of two sums 1e6 times larger, 1.2e-12 ...
ERROR_FORM_ERROR = 1.3e-12
TIE = 100.0 * ERROR_FORM_ERROR           # ... and the margin below which a line-search decision counts as a tie


class NotFitted(Exception):
    """The Gram route declines (status 1)."""


# --------------------------------------------------------------------------- the data form (the reference restated)
def _project_psd(Q, lo=0.0, hi=math.inf):
    lam, V = np.linalg.eigh((Q + Q.T) / 2)
    return (V * np.minimum(hi, np.maximum(lam, lo))) @ V.T


def _polar(M):
    """(U, P) with M = U P, U orthogonal, P symmetric positive semi-definite, by the SVD."""
    W, s, Vh = np.linalg.svd(M)
    return W @ Vh, (Vh.T * s) @ Vh


def _data_error(Xs, Xu, Y, S, U, B, Bcon, grads=True):
    Sinv = np.linalg.inv(S)
    R = Sinv @ U @ B @ S
    E = Y - Bcon @ Xu - R @ Xs
    e = np.linalg.norm(E, "fro")
    if not grads:
        return e
    t1 = Sinv.T @ (-E) @ Xs.T
    return e, -t1 @ R.T + B.T @ U.T @ t1, t1 @ S.T @ B.T, U.T @ t1 @ S.T, -E @ Xu.T


def _fgm(ops, S, U, B, Bcon, cond, norm_y, stats):
    """The fast-gradient loop of stabilize_discrete (stable_koopman.py:73-165) over abstract operations: ops.error(it)
    -> e, ops.grads(it) -> (gS, gU, gB, gBcon), ops.project(Ys, Yu, Yb, Ybc, g, step) -> it (an iterate: a dict with S,
    U, B, Bcon, cond and whatever the operations keep with it).  Returns the final iterate and error; stats gains
    iterations (outer loop bodies run), trials and margin (the smallest relative distance of a decision from its
    threshold)."""
    cur = ops.start(S, U, B, Bcon, cond)
    error = ops.error(cur)
    step = 1.0 / (cur["cond"] * cur["cond"])
    i, alpha, restarti, inner0 = 1, ALPHA0, 1, 1
    Ys, Yu, Yb, Ybc = cur["S"], cur["U"], cur["B"], cur["Bcon"]
    stats.update(iterations=0, trials=0, margin=math.inf)
    while i < MAX_OUTER:
        stats["iterations"] += 1
        g = ops.grads(cur)
        error_next, inner = math.inf, 1
        step *= 2
        ops.current = error                                  # (what the trials' errors are compared with: for logs)
        nxt = None
        while error_next > error and ((i == 1 and inner <= LS_MAX_FIRST) or inner <= LS_MAX):
            nxt = ops.project(Ys, Yu, Yb, Ybc, g, step)
            error_next = ops.error(nxt)
            stats["trials"] += 1
            if error > 0:
                stats["margin"] = min(stats["margin"], abs(error_next - error) / error)
            step /= LS_PARAM
            inner += 1
        if i == 1:
            inner0 = inner
        alpha_next = (math.sqrt(alpha ** 4 + 4 * alpha ** 2) - alpha ** 2) / 2
        beta = alpha * (1 - alpha) / (alpha ** 2 + alpha_next)
        if inner >= LS_MAX + 1:                              # the line search failed
            if restarti == 1:                                # restart the FGM from the current iterate
                restarti = 0
                alpha_next = ALPHA0
                Ys, Yu, Yb, Ybc = cur["S"], cur["U"], cur["B"], cur["Bcon"]
                error_next = error
                shrink = 1.0                                 # LS_PARAM ** inner0, by multiplication as on the device
                for _ in range(inner0):
                    shrink *= LS_PARAM
                step = 1.0 / (cur["cond"] * cur["cond"]) / shrink
            else:
                break
        else:
            restarti = 1
            Ys = nxt["S"] + beta * (nxt["S"] - cur["S"])
            Yu = nxt["U"] + beta * (nxt["U"] - cur["U"])
            Yb = nxt["B"] + beta * (nxt["B"] - cur["B"])
            Ybc = nxt["Bcon"] + beta * (nxt["Bcon"] - cur["Bcon"])
            cur = nxt
        i += 1
        error, alpha = error_next, alpha_next
        thr = CONVERGED * norm_y
        if thr > 0:
            stats["margin"] = min(stats["margin"], abs(error - thr) / thr)
        if error < thr:
            break
    return cur, error


class _DataOps:
    def __init__(self, Xs, Xu, Y, log=None):
        self.d, self.log = (Xs, Xu, Y), log

    def start(self, S, U, B, Bcon, cond):
        return {"S": S, "U": U, "B": B, "Bcon": Bcon, "cond": cond}

    def error(self, it):
        e = _data_error(*self.d, it["S"], it["U"], it["B"], it["Bcon"], grads=False)
        if self.log is not None:
            self.log.append(e)
        return e

    def grads(self, it):
        return _data_error(*self.d, it["S"], it["U"], it["B"], it["Bcon"])[1:]

    def project(self, Ys, Yu, Yb, Ybc, g, step):
        S = _project_psd(Ys - g[0] * step, S_FLOOR)
        lam = np.linalg.eigvalsh(S)
        return {"S": S, "U": _polar(Yu - g[1] * step)[0], "B": _project_psd(Yb - g[2] * step, 0.0, 1.0),
                "Bcon": Ybc - g[3] * step, "cond": np.max(lam) / np.min(lam)}


def stabilize_host(Xs, Xu, Y, stats=None):
    """``stabilize_discrete(Xs, Xu, Y)`` of the reference with its default initialisation (S = I, [U, B] the polar
    decomposition of the least-squares A, B clipped to [0, 1]), restated: Xs [n][m], Xu [nu][m], Y [n][m].  Returns
    (A, Bcon, error); stats, a dict, receives iterations, trials and margin."""
    Xs, Xu, Y = (np.asarray(a, dtype=np.float64) for a in (Xs, Xu, Y))
    n = Xs.shape[0]
    W0 = Y @ np.linalg.pinv(np.vstack((Xs, Xu)))
    U, B = _polar(W0[:n, :n])
    B = _project_psd(B, 0.0, 1.0)
    stats = {} if stats is None else stats
    it, error = _fgm(_DataOps(Xs, Xu, Y), np.identity(n), U, B, W0[:n, n:], 1.0, np.linalg.norm(Y, "fro"), stats)
    A = np.linalg.inv(it["S"]) @ it["U"] @ it["B"] @ it["S"]
    return A, it["Bcon"], float(error)


def koopman_rows(lens, obs, ctrls, basis):
    """(Xs [n][m], Xu [nu][m], Y [n][m]) of a Koopman basis, as ``Koopman.train`` forms them."""
    _, valid = _row_start(np.asarray(lens, dtype=np.int64))
    g = np.nonzero(valid)[0]
    Z = lift(np.asarray(obs, dtype=np.float64), basis)
    return Z[g].T, np.asarray(ctrls, dtype=np.float64)[g].T, Z[g + 1].T


# --------------------------------------------------------------------------------------------------- the Gram form
def jacobi_pairs(m, r):
    """The m / 2 disjoint pairs (p < q) of round r (0 .. m - 2) of the round-robin order on m (even) indices: index
    m - 1 meets r, and (r + k) mod (m - 1) meets (r - k) mod (m - 1), k = 1 .. m / 2 - 1."""
    k = np.arange(1, m // 2)
    a = np.concatenate([[m - 1], (r + k) % (m - 1)])
    b = np.concatenate([[r], (r - k) % (m - 1)])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi_eigh(A, sweeps=JACOBI_SWEEPS):
    """(lam, V, sweeps run) of a symmetric matrix by two-sided cyclic Jacobi in the parallel order of jacobi_pairs,
    the device's eigensolver step for step: per round the n / 2 rotations are computed from the current matrix and
    applied together, A <- J'AJ on 2 x 2 blocks, V <- V J.  A pair is rotated when |a_pq| > JACOBI_EPS (|a_pp| +
    |a_qq|); the iteration ends after a sweep without rotation.  Raises NotFitted at the sweep cap.  The eigenvalues
    come unsorted."""
    n = A.shape[0]
    m = n + (n & 1)
    W = np.zeros((m, m))
    W[:n, :n] = A
    V = np.identity(m)
    for sweep in range(sweeps):
        rotated = False
        for r in range(m - 1):
            p, q = jacobi_pairs(m, r)
            app, aqq, apq = W[p, p], W[q, q], W[p, q]
            rot = np.abs(apq) > JACOBI_EPS * (np.abs(app) + np.abs(aqq))
            if not rot.any():
                continue
            rotated = True
            with np.errstate(all="ignore"):
                tau = (aqq - app) / (2.0 * np.where(rot, apq, 1.0))
                t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
            t = np.where(rot, t, 0.0)
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = t * c
            # rows: W <- J'W
            Wp, Wq = W[p, :].copy(), W[q, :].copy()
            W[p, :], W[q, :] = c[:, None] * Wp - s[:, None] * Wq, s[:, None] * Wp + c[:, None] * Wq
            # columns: W <- W J
            Wp, Wq = W[:, p].copy(), W[:, q].copy()
            W[:, p], W[:, q] = c[None, :] * Wp - s[None, :] * Wq, s[None, :] * Wp + c[None, :] * Wq
            W[p[rot], q[rot]] = 0.0
            W[q[rot], p[rot]] = 0.0
            Vp, Vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c[None, :] * Vp - s[None, :] * Vq, s[None, :] * Vp + c[None, :] * Vq
        if not rotated:
            return np.diagonal(W)[:n].copy(), V[:n, :n], sweep + 1
    raise NotFitted("Jacobi sweep cap")


def _eigh(A, eig):
    if eig == "jacobi":
        lam, V, _ = jacobi_eigh(A)
        return lam, V
    return np.linalg.eigh(A)


def _spectral(V, f):
    return (V * f) @ V.T


def _gram_polar(M, eig):
    """(the polar factor of M, eigenvalues of M'M, V): M (M'M)^-1/2, then two Newton-Schulz steps U <- U (3 I - U'U) / 2,
    which take a departure from orthogonality d to about d^4."""
    lam, V = _eigh(M.T @ M, eig)
    if not (np.all(np.isfinite(lam)) and np.min(lam) > POLAR_EPS * np.max(lam)):
        raise NotFitted("polar factor")
    U = M @ _spectral(V, 1.0 / np.sqrt(lam))
    for _ in range(2):
        U = U @ (1.5 * np.identity(len(U)) - 0.5 * (U.T @ U))
    return U, lam, V


class _GramOps:
    def __init__(self, G, W0, e0sq, eig, log=None):
        self.G, self.W0, self.e0sq, self.eig, self.log = G, W0, e0sq, eig, log
        self.n = W0.shape[0]

    def start(self, S, U, B, Bcon, cond):
        return self._finish({"S": S, "U": U, "B": B, "Bcon": Bcon, "cond": cond, "Sinv": np.linalg.inv(S)})

    def _finish(self, it):
        it["R"] = it["Sinv"] @ (it["U"] @ (it["B"] @ it["S"]))
        D = np.concatenate([it["R"], it["Bcon"]], axis=1) - self.W0
        it["T"] = D @ self.G
        it["e"] = math.sqrt(max(self.e0sq + float(np.sum(it["T"] * D)), 0.0))
        if not np.isfinite(it["e"]):
            raise NotFitted("not finite")
        return it

    def error(self, it):
        if self.log is not None:
            self.log.append((it["e"], it, getattr(self, "current", None)))
        return it["e"]

    def grads(self, it):
        n = self.n
        t1 = it["Sinv"] @ it["T"][:, :n]
        x1, x2 = t1 @ it["S"], it["U"].T @ t1
        return it["B"] @ x2 - t1 @ it["R"].T, x1 @ it["B"], it["U"].T @ x1, it["T"][:, n:]

    def project(self, Ys, Yu, Yb, Ybc, g, step):
        X = Ys - g[0] * step
        lam, V = _eigh((X + X.T) / 2, self.eig)
        lam = np.maximum(lam, S_FLOOR)
        it = {"S": _spectral(V, lam), "Sinv": _spectral(V, 1.0 / lam), "cond": np.max(lam) / np.min(lam)}
        it["U"] = _gram_polar(Yu - g[1] * step, self.eig)[0]
        X = Yb - g[2] * step
        lam, V = _eigh((X + X.T) / 2, self.eig)
        it["B"] = _spectral(V, np.minimum(1.0, np.maximum(lam, 0.0)))
        it["Bcon"] = Ybc - g[3] * step
        return self._finish(it)


def design_gram(lens, obs, ctrls, basis):
    """(G [nf][nf], Q [nf][nt], yy [nt]) of one basis: the uncentred Gram of [F | Y] summed over blocks of SPLIT_ROWS
    data rows in order (the device's row splits); of Y'Y the diagonal only."""
    _, valid = _row_start(lens)
    Z = lift(obs, basis)
    nt, nf = Z.shape[1], Z.shape[1] + ctrls.shape[1]
    raw, yy = np.zeros((nf, nf + nt)), np.zeros(nt)
    for r0 in range(0, obs.shape[0], SPLIT_ROWS):
        g = r0 + np.nonzero(valid[r0:r0 + SPLIT_ROWS])[0]
        if not len(g):
            continue
        D = np.concatenate([Z[g], ctrls[g], Z[g + 1]], axis=1)
        raw += D[:, :nf].T @ D
        yy += np.sum(D[:, nf:] * D[:, nf:], axis=0)
    FF = raw[:, :nf]
    return np.triu(FF) + np.triu(FF, 1).T, raw[:, nf:].copy(), yy


def fgm_on_gram(G, Q, yy, tie=TIE, eig="lapack", log=None, perturb=None):
    """The recursion of the module docstring on one Gram.  Returns (coeffs [n][n + nu] or NaN, status, error,
    iterations, trials, margin).  log, a list, receives (e, iterate, the error it is compared with -- None at the start) of every error evaluation; perturb(G, Q, yy)
    may return a changed Gram (the round-off response of the goldens)."""
    nf, n = Q.shape
    nan = (np.full((n, nf), np.nan), 1, math.nan, 0, 0, math.inf)
    if perturb is not None:
        G, Q, yy = perturb(G, Q, yy)
    GQ = np.concatenate([G, Q], axis=1)
    if not np.all(np.isfinite(GQ)) or not np.all(np.isfinite(yy)):
        return nan
    W0, bad, _ = solve_scaled_cholesky(GQ, np.arange(nf), nf, n)
    if bad:
        return nan
    e0sq = max(float(np.sum(yy)) - float(np.sum(W0 * Q.T)), 0.0)
    stats = {}
    try:
        U, lam, V = _gram_polar(W0[:, :n], eig)
        B = _spectral(V, np.minimum(1.0, np.sqrt(lam)))
        it, error = _fgm(_GramOps(G, W0, e0sq, eig, log), np.identity(n), U, B, W0[:, n:].copy(), 1.0,
                         math.sqrt(float(np.sum(yy))), stats)
    except NotFitted:
        return nan
    coef = np.concatenate([it["R"], it["Bcon"]], axis=1)
    if not (np.all(np.isfinite(coef)) and np.isfinite(error)):
        return nan
    return (coef, 2 if stats["margin"] <= tie else 0, float(error), stats["iterations"], stats["trials"],
            stats["margin"])


def stable_fit_host(traj_len, obs, ctrls, bases, tie=TIE, eig="lapack", log=None, perturb=None):
    """``_lib.stable_fit`` in numpy.  bases: (kinds, params) pairs, one configuration each.  Returns (coeffs, status,
    error, iterations, trials, min_margin): a list of [n][n + nu] matrices ``[A | B]`` and five per-basis arrays."""
    lens = np.asarray(traj_len, dtype=np.int64)
    obs, ctrls = np.asarray(obs, dtype=np.float64), np.asarray(ctrls, dtype=np.float64)
    out = []
    for kinds, params in bases:
        key = (tuple(int(k) for k in kinds), tuple(float(p) for p in params))
        out.append(fgm_on_gram(*design_gram(lens, obs, ctrls, key), tie=tie, eig=eig, log=log, perturb=perturb))
    return ([o[0] for o in out], np.array([o[1] for o in out], dtype=np.int32),
            np.array([o[2] for o in out], dtype=np.float64), np.array([o[3] for o in out], dtype=np.int32),
            np.array([o[4] for o in out], dtype=np.int32), np.array([o[5] for o in out], dtype=np.float64))
