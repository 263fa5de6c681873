"""Shared by the SINDy-fit tests: seeded training data, the configurations, and per case (computed once) the model's
own ``train()`` result and the numpy restatement's (``stlsq_gram_host``)."""
import functools

import numpy as np

from autompc_amd import SINDy
from autompc_amd.sysid import sindy_fit as SF
from autompc_amd.sysid.linear_fit import concat_trajs
from autompc_amd.sysid.sindy import build_library
from linfit_cases import make_trajs, system

CONFIGS = {
    1: dict(),
    2: dict(threshold=0.05),
    3: dict(trig_basis=True, trig_freq=1, threshold=0.02),
    4: dict(trig_basis=True, trig_freq=2, trig_interaction=True, threshold=0.02),
    5: dict(poly_basis=True, poly_degree=3, threshold=0.01),
    6: dict(poly_basis=True, poly_degree=3, poly_cross_terms=True, threshold=0.02),
    7: dict(trig_basis=True, trig_freq=2, time_mode="continuous", threshold=0.1),
    8: dict(poly_basis=True, poly_degree=5, trig_basis=True, trig_freq=3, threshold=0.03),
    9: dict(threshold=5.0),                    # everything is eliminated
}
# name -> ((obs_dim, ctrl_dim), trajectory lengths); "long": three row splits, boundaries 512 and 1024 inside a
# trajectory, a length-1 trajectory (discrete mode only: np.gradient needs two rows).  "wide": the device's state and
# control limits.  "edges" (1057 rows, discrete mode only): a trajectory ends on row 511, the split of rows 512 .. 1023
# holds 512 one-row trajectories and so no design row, R % 16 == 1 and the lone last row has no successor.
DATA = {"small": ((3, 1), [40, 17, 64, 33, 90, 2, 3, 25]), "hc": ((17, 6), [80] * 12),
        "long": ((3, 1), [300, 1, 500, 400]), "wide": ((64, 16), [60] * 10),
        "edges": ((3, 1), [512] + [1] * 512 + [2, 30, 1])}
# every device-eligible case; configurations 4 and 6 have 2139 / 2599 features on 17 / 6 ("size")
ELIGIBLE = [("small", k) for k in sorted(CONFIGS)] + [("hc", k) for k in (1, 2, 3, 5, 7, 8, 9)]
LONG = [("long", k) for k in (1, 3, 5, 8)]
EDGES = [("edges", k) for k in (1, 3, 5)]
FEATURES = {("small", 1): 4, ("small", 4): 68, ("hc", 1): 23, ("hc", 3): 69, ("hc", 7): 115, ("hc", 8): 253,
            ("hc", 4): 2139, ("hc", 6): 2599}

# Cases on libraries the stock constructor does not yield: the first n features of a build_library result
# (LIBRARIES: its arguments after the variable count), optionally with feature `dup` appended a second time.  A case
# is dict(library=(name, n[, dup]), threshold=..[, time_mode=..][, alpha=..]); a key (k, alpha) is case k at that
# ridge alpha (alpha belongs to the call: the cases of one request must agree on it).
LIBRARIES = {"id": dict(), "trig1": dict(trig_freq=1), "trig2": dict(trig_freq=2),
             "trig2x": dict(trig_freq=2, trig_interaction=True), "trig4pow4": dict(trig_freq=4, poly_degree=4),
             "trig3pow6": dict(trig_freq=3, poly_degree=6), "pow4": dict(poly_degree=4)}
EDGE_CONFIGS = {}
for _lib_name, _ns, _thr in (("trig2", (1, 15, 16, 17), 0.02), ("trig2x", (31, 32, 33), 0.02),
                             ("trig4pow4", (255, 256, 257, 271, 272), 0.03), ("trig3pow6", (272,), 0.03),
                             ("pow4", (272,), 0.03)):
    for _n in _ns:
        EDGE_CONFIGS["%s:%d" % (_lib_name, _n)] = dict(library=(_lib_name, _n), threshold=_thr)
EDGE_CONFIGS.update({
    "trig4pow4:1": dict(library=("trig4pow4", 1), threshold=0.03),
    "trig4pow4:16": dict(library=("trig4pow4", 16), threshold=0.03),
    "trig1:240": dict(library=("trig1", 240), threshold=0.03),
    "trig1:240c": dict(library=("trig1", 240), threshold=0.03, time_mode="continuous"),
    "7d": dict(CONFIGS[7], time_mode="discrete", threshold=0.02),          # configuration 7's library, discrete
    # library D: configuration 3's with feature 5 (sin x1) a second time; singular without the ridge
    "dup": dict(library=("trig1", 12, 5), threshold=0.02),
    # the states alone (no control column), both target sets
    "states": dict(library=("id", 3), threshold=0.02),
    "states_c": dict(library=("id", 3), threshold=0.1, time_mode="continuous"),
    # the plain library, the threshold between the largest and the second largest |coef| of every target's first
    # solve on "small" (0.97 | 0.44, 1.01 | 0.088, 0.97 | 0.34): every second solve keeps one feature
    "kept1": dict(threshold=0.6),
})
# feature counts at the 16-column tile edges (nf % 16 == 0: nfp == nf and the targets start a tile of their own) and
# nf = 1 (no back substitution)
EDGE_SMALL = [("small", "trig2:%d" % n) for n in (1, 15, 16, 17)] + [("small", "trig2x:%d" % n) for n in (31, 32, 33)]
# both sides of the solve kernel's 256 threads and the 272-feature limit; "trig3pow6:272" is the case nearest the
# pivot line (10 x)
EDGE_WIDE = [("hc", "trig4pow4:%d" % n) for n in (255, 256, 257, 271, 272)] + [("hc", "trig3pow6:272")]
# 64 states, 16 controls: 64 solve workgroups per configuration; 240 + 2 x 64 = 368 columns when one design carries
# both target sets
LIMITS = [("wide", "trig1:240"), ("wide", "trig1:240c"), ("wide", "pow4:272")]
# The later solves of the tables above keep 8 and 9 features (both sides of the Cholesky panel width) but never 1 (the
# back substitution's degenerate case): "kept1" does.
EDGE_KEPT = [("small", "kept1")]
# designs of 1, 16, 257 and 272 features and the plain 23 in one launch
EXTREMES = [("hc", "trig4pow4:%d" % n) for n in (1, 16, 257, 272)] + [("hc", 1)]
# one design with both target sets (discrete, continuous), also on a caller's xdot
BOTH = [("wide", "trig1:240", "trig1:240c"), ("small", "7d", 7)]
# the good neighbours of the declining configurations, at the declining call's alpha
NEIGHBOURS = {0.0: [("small", (1, 0.0)), ("small", (5, 0.0))], 1e-9: [("small", (1, 1e-9)), ("small", (5, 1e-9))]}
ALPHAS = [("small", (3, 0.0)), ("small", (3, 10.0))]


def config(k):
    """The case dictionary of a key: a CONFIGS number, an EDGE_CONFIGS name, or (key, alpha)."""
    if isinstance(k, tuple):
        return dict(config(k[0]), alpha=float(k[1]))
    return dict(CONFIGS[k] if k in CONFIGS else EDGE_CONFIGS[k])


def alpha_of(k):
    return config(k).get("alpha", 0.05)


def first_features(lib, n):
    """The first n feature descriptors of a build_library result (the two pair arrays are kept whole)."""
    if not 1 <= n <= len(lib[0]):
        raise ValueError("the library has %d features" % len(lib[0]))
    return tuple(a[:n].copy() for a in lib[:4]) + tuple(lib[4:])


def with_duplicate(lib, i):
    """`lib` with feature i appended a second time."""
    return tuple(np.append(a, a[i]) for a in lib[:4]) + tuple(lib[4:])


@functools.lru_cache(maxsize=None)
def library(name, lib, n, dup=None):
    s = data(name)[0]
    out = first_features(build_library(s.obs_dim + s.ctrl_dim, **LIBRARIES[lib]), n)
    return out if dup is None else with_duplicate(out, dup)


@functools.lru_cache(maxsize=None)
def data(name):
    """(system, trajectories) of a data set."""
    shape, lens = DATA[name]
    s = system(*shape)
    return s, make_trajs(s, lens, seed=5)


def new_model(name, k, **kw):
    cfg = dict(config(k), **kw)
    lib = cfg.pop("library", None)
    cfg.pop("alpha", None)
    m = SINDy(data(name)[0], **cfg)
    if lib is not None:
        m.library = library(name, *lib)
        m.coefficients = np.zeros((m.system.obs_dim, len(m.library[0])))
    return m


@functools.lru_cache(maxsize=None)
def caller_xdot(name):
    """A caller's xdot for a data set: seeded normal values, one [len][nx] array per trajectory."""
    rng = np.random.default_rng(1)
    return [rng.normal(size=t.obs.shape) for t in data(name)[1]]


@functools.lru_cache(maxsize=None)
def trained(name, k, xdot=False):
    """Coefficients after the model's own train() (at the case's alpha; `xdot`: on caller_xdot)."""
    m = new_model(name, k)
    m.train(data(name)[1], xdot=caller_xdot(name) if xdot else None, alpha=alpha_of(k))
    return m.coefficients


def request(name, ks, xdot=False):
    """Arguments of ``_lib.sindy_fit`` / ``stlsq_gram_host`` for configurations `ks` of one data set: models of equal
    libraries share a design.  The cases' alpha enters the keyword arguments when it is not the default."""
    s, trajs = data(name)
    lens, obs, ctrls = concat_trajs(trajs)
    designs, index, configs = [], {}, []
    for k in ks:
        m = new_model(name, k)
        key = SF._library_key(m)
        if key not in index:
            index[key] = len(designs)
            designs.append(m.library)
        configs.append((index[key], m.time_mode == "continuous", m.threshold))
    ycont = None
    if any(c[1] for c in configs):
        ycont = SF.continuous_targets(trajs, s.dt, caller_xdot(name) if xdot else None)
    alphas = {alpha_of(k) for k in ks}
    if len(alphas) != 1:
        raise ValueError("the cases of one request must share alpha")
    alpha = alphas.pop()
    return (lens, obs, ctrls, designs, configs), dict(dict(ycont=ycont), **({} if alpha == 0.05 else {"alpha": alpha}))


@functools.lru_cache(maxsize=None)
def host_fit(name, k, xdot=False):
    """(coefficients, status, pivot, margin, iterations) of stlsq_gram_host for one case."""
    args, kw = request(name, [k], xdot)
    c, st, piv, mar, it = SF.stlsq_gram_host(*args, **kw)
    return c[0], int(st[0]), float(piv[0]), float(mar[0]), int(it[0])


def rel_err(a, ref):
    """max|d| / max|coef| (the plain largest difference when the reference is all zero)."""
    den = float(np.max(np.abs(ref)))
    return float(np.max(np.abs(np.asarray(a) - ref))) / (den if den > 0 else 1.0)


def same_support(a, ref):
    return np.array_equal(np.asarray(a) != 0, np.asarray(ref) != 0)
