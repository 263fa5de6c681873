"""Shared by the wide SINDy-fit tests (libraries of 273..2048 features): data, libraries, targets and per case
(computed once) the model's own ``train()`` result and the numpy restatement's (``stlsq_gram_host``).

Data.  Few variables, observations and controls drawn i.i.d. uniform over [-pi, pi]: trig features of distinct integer
frequency are then orthogonal in expectation, and with at least 3 design rows per feature the unit-diagonal Gram's
smallest eigenvalue stays near (1 - sqrt(1/3))^2 = 0.18, far from the pivot line.  Targets.  Every case is a
continuous-mode configuration on a caller's ``xdot`` made for the case: ``Theta[:, idx] w + 1e-3 noise`` with a handful
of coefficients ``w`` of size 0.5 .. 2 and threshold 0.1, so the first solve drops all but ``idx`` (the other
coefficients are at noise level, far below the threshold) and the second solve, on ``len(idx)`` features, is the last.
The discrete targets of such data (the next observation) are noise: a discrete configuration here has threshold 0 and
one solve.
"""
import contextlib
import functools

import numpy as np

from autompc_amd import SINDy
from autompc_amd.sysid import sindy_fit as SF
from autompc_amd.sysid.linear_fit import concat_trajs
from autompc_amd.sysid.sindy import _features, build_library
from autompc_amd.trajectory import Trajectory
from linfit_cases import system
from sindy_fit_cases import first_features, rel_err, same_support, with_duplicate     # noqa: F401

PANEL = 32                 # the wide solve's panel width (kWideNb)
GROUP = 128                # columns of one wave's run of tiles in the wide Gram pass (kWideAcc * 16)
THETA_BLOCK = 256          # columns per workgroup of the kernel that materialises [Theta | Y]
THRESHOLD = 0.1

# name -> ((obs_dim, ctrl_dim), trajectory lengths, build_library arguments after the variable count)
# "s": 1598 design rows in 4 row splits, libraries of up to 525 features; "big": 6199 design rows in 13 splits, up to
# 2050 features; "edges" (1057 rows): the narrow tests' edge layout -- a trajectory ends on row 511, the split of rows
# 512 .. 1023 holds 512 one-row trajectories and so no design row, the lone last row has no successor; 541 design rows
DATA = {"s": ((2, 1), [900, 700], dict(trig_freq=29, trig_interaction=True)),
        "big": ((1, 1), [6200], dict(trig_freq=256, trig_interaction=True)),
        "edges": ((2, 1), [512] + [1] * 512 + [2, 30, 1], dict(trig_freq=29, trig_interaction=True))}

# feature counts, each alone in its call: the first past the narrow limit; around multiples of the panel width, of a
# wave's tile run and of the Theta kernel's column block (the smallest multiples past 272); the narrow sizes through
# the wide entry; the limit
COUNTS_S = [1, 17, 272, 273, PANEL * 9 - 1, PANEL * 9, PANEL * 9 + 1, GROUP * 3 - 1, GROUP * 3, GROUP * 3 + 1,
            THETA_BLOCK * 2 - 1, THETA_BLOCK * 2, THETA_BLOCK * 2 + 1]
COUNTS_BIG = [2047, 2048]
SIZES = [("s", n) for n in COUNTS_S] + [("big", n) for n in COUNTS_BIG]
# the second solve keeps one feature / 33 (one past a panel edge)
SHRINK = [("s", 300, 1), ("s", 300, PANEL + 1)]
MIXED = [("s", 273), ("s", 400), ("s", 513)]       # designs of different widths in one launch (+ ("big", 2048) alone)
EDGE_ROWS = [("edges", 17), ("edges", 180)]


@functools.lru_cache(maxsize=None)
def data(name):
    """(system, trajectories) of a data set."""
    shape, lens, _ = DATA[name]
    s = system(*shape)
    rng = np.random.default_rng(7)
    return s, [Trajectory(s, T, rng.uniform(-np.pi, np.pi, size=(T, shape[0])),
                          rng.uniform(-np.pi, np.pi, size=(T, shape[1]))) for T in lens]


@functools.lru_cache(maxsize=None)
def full_library(name):
    shape, _, kw = DATA[name]
    return build_library(shape[0] + shape[1], **kw)


def library(name, n):
    return first_features(full_library(name), n)


def support_of(n, kept=None):
    """The features with a true coefficient: `kept` of them spread over the library (default: up to five)."""
    if kept is None:
        return sorted({0, n // 7, n // 3, n // 2, n - 1})
    return sorted({int(round(i * (n - 1) / max(kept - 1, 1))) for i in range(kept)})


@functools.lru_cache(maxsize=None)
def xdot(name, n, kept=None):
    """The caller's xdot of a case, one [len][nx] array per trajectory (module docstring)."""
    s, trajs = data(name)
    lib, idx = library(name, n), support_of(n, kept)
    rng = np.random.default_rng(100 + n + (kept or 0))
    w = rng.uniform(0.5, 2.0, size=(len(idx), s.obs_dim)) * rng.choice([-1.0, 1.0], size=(len(idx), s.obs_dim))
    sub = tuple(a[idx] for a in lib[:4]) + tuple(lib[4:])
    out = []
    for t in trajs:
        out.append(_features(sub, np.concatenate([t.obs, t.ctrls], axis=1)) @ w
                   + 1e-3 * rng.normal(size=(len(t), s.obs_dim)))
    return out


def new_model(name, lib, threshold=THRESHOLD, time_mode="continuous"):
    m = SINDy(data(name)[0], threshold=threshold, time_mode=time_mode)
    m.library = lib
    m.coefficients = np.zeros((m.system.obs_dim, len(lib[0])))
    return m


def request(name, n, kept=None, threshold=THRESHOLD):
    """Arguments of ``_lib.sindy_fit_wide`` / ``stlsq_gram_host`` for the case alone."""
    s, trajs = data(name)
    lens, obs, ctrls = concat_trajs(trajs)
    ycont = SF.continuous_targets(trajs, s.dt, xdot(name, n, kept))
    return (lens, obs, ctrls, [library(name, n)], [(0, True, threshold)]), dict(ycont=ycont)


@functools.lru_cache(maxsize=None)
def trained(name, n, kept=None):
    m = new_model(name, library(name, n))
    m.train(data(name)[1], xdot=xdot(name, n, kept))
    return m.coefficients


def scaled_cholesky_blocked(S, b, nb=64):
    """``SF._scaled_cholesky_1`` with the trailing update done per panel of `nb` columns as one matrix product: the same
    scaled right-looking factorisation (the right-hand side carried as an extra row) without the python loop over every
    column's rank-1 update.  Returns (w or None, smallest squared pivot)."""
    n = len(b)
    diag = np.diag(S)
    if not (np.all(diag > 0) and np.all(np.isfinite(diag))):
        return None, float(np.min(diag))
    d = 1.0 / np.sqrt(diag)
    M = np.empty((n + 1, n))
    M[:n] = S * d[:, None] * d[None, :]
    M[n] = b * d
    minp = np.inf
    for j0 in range(0, n, nb):
        j1 = min(j0 + nb, n)
        for j in range(j0, j1):
            p = M[j, j]
            if not (p > 0 and np.isfinite(p)):
                return None, float(p)
            minp = min(minp, p)
            M[j, j] = np.sqrt(p)
            M[j + 1:, j] /= M[j, j]
            M[j + 1:, j + 1:j1] -= np.multiply.outer(M[j + 1:, j], M[j + 1:j1, j])
        M[j1:, j1:] -= M[j1:, j0:j1] @ M[j1:n, j0:j1].T
    y = M[n]
    for j in range(n - 1, -1, -1):
        y[j] /= M[j, j]
        y[:j] -= y[j] * M[j, :j]
    return y * d, float(minp)


@contextlib.contextmanager
def blocked_host():
    """``stlsq_gram_host`` on the blocked factorisation (for the cases too wide for the python loop)."""
    plain = SF._scaled_cholesky_1
    SF._scaled_cholesky_1 = scaled_cholesky_blocked
    try:
        yield
    finally:
        SF._scaled_cholesky_1 = plain


def host_call(args, kw):
    """stlsq_gram_host of a request; the blocked factorisation when a design is wider than 600 features."""
    if max(len(d[0]) for d in args[3]) > 600:
        with blocked_host():
            return SF.stlsq_gram_host(*args, **kw)
    return SF.stlsq_gram_host(*args, **kw)


@functools.lru_cache(maxsize=None)
def host_fit(name, n, kept=None):
    """(coefficients, status, pivot, margin, iterations) of stlsq_gram_host for one case."""
    c, st, piv, mar, it = host_call(*request(name, n, kept))
    return c[0], int(st[0]), float(piv[0]), float(mar[0]), int(it[0])


def only_states(lib, nx):
    """The features of `lib` that read no control (variables below nx); not for monomial features."""
    keep = (lib[1] < nx) & (lib[2] < nx)
    return tuple(a[keep] for a in lib[:4]) + tuple(lib[4:])
