"""Shared by the lasso-fit tests: the cases of tests/golden/gen_golden_lassofit.py (the reference's own
Koopman(method="lasso").train on each) and the models that go with them."""
import functools
import os

import numpy as np

from autompc_amd import Koopman, Trajectory
from autompc_amd.sysid import lasso_fit as LS

from linfit_cases import make_trajs, system

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FOUR_LIFTS = dict(strict_reference=False, poly_basis=True, poly_degree=2, trig_basis=True, trig_freq=1)
# raw bases (kinds, params): 0 = x, 1 = x^p, 2 = sin px, 3 = cos px
TWO, FOUR = ([0, 1], [1.0, 2.0]), ([0, 1, 2, 3], [1.0, 2.0, 1.0, 1.0])
# 606 data rows, two row splits of 512: the 270-row trajectory ends on data row 511, the last row of split 0; a
# length-1 trajectory opens split 1 and another closes the data; 597 design rows
RAGGED = [1, 40, 1, 200, 270, 1, 90, 2, 1]
# name -> observations, controls, trajectory lengths, data seed, Koopman arguments ("koopman") or a raw basis
# ("basis"), lasso alphas, and what is done to the data: "hold" (control column, value it is held at), "zero_obs"
# (observation columns set to 0), "jitter" (control column, c, s): replaced by c (1 + s N(0, 1)), drawn from seed + 1
CASES = {
    # 13 features (x, x^2, sin x, cos x of 3 observations + 1 control), 234 rows: alpha 1e2 zeroes every coefficient
    # in one sweep, 1e-6 runs every target into the 1000-sweep cap
    "n13": dict(no=3, nu=1, lengths=[40] * 6, seed=301, koopman=FOUR_LIFTS, alphas=(1e2, 1.0, 1e-2, 1e-6), hold=None),
    # the strict-reference basis of poly_degree 3 with trig: x, x^3 twice, (sin 3x, cos 3x) three times: 19 features
    "dup": dict(no=2, nu=1, lengths=[30] * 5, seed=302, koopman=dict(poly_basis=True, poly_degree=3, trig_basis=True),
                alphas=(1e-1, 1e-5), hold=None),
    # 74 features: more than one wave's 64 lanes; the alpha converges within a few dozen sweeps
    "n74": dict(no=17, nu=6, lengths=[50] * 6, seed=303, koopman=FOUR_LIFTS, alphas=(1e-1,), hold=None),
    # the largest design: 256 lifted states + 16 controls
    "big": dict(no=64, nu=16, lengths=[31] * 10, seed=304, koopman=FOUR_LIFTS, alphas=(1.0,), hold=None),
    # a control column that is identically zero: never updated, coefficient 0, still fitted on the Gram route
    "zero": dict(no=3, nu=2, lengths=[40] * 4, seed=305, koopman=dict(poly_basis=True, poly_degree=2),
                 alphas=(1e-3,), hold=(1, 0.0)),
    # a control column held at 0.75: its centred sum of squares is rounding noise -> status 1 -> train()
    "const": dict(no=3, nu=2, lengths=[40] * 4, seed=306, koopman=dict(poly_basis=True, poly_degree=2),
                  alphas=(1e-3,), hold=(1, 0.75)),
}


def _ragged(no, nu, lifts, seed, alpha=1e-1, **change):
    return dict(no=no, nu=nu, lengths=RAGGED, seed=seed, basis=lifts, alphas=(alpha,), hold=None, **change)


# the feature counts at which lasso_cd_kernel's lane / slot addressing changes, on the ragged two-split data
SWEEP = {
    "s15": _ragged(7, 1, TWO, 7006),        # 1 + nf = 16: Y starts on a tile edge; wp is one pad short of 32
    "s63": _ragged(31, 1, TWO, 7001),       # 1 + nf = 64; lane 63 is the last feature
    "s64": _ragged(12, 16, FOUR, 7002),     # ldp == nf, 16 controls
    "s65": _ragged(16, 1, FOUR, 7003),      # slot 1 holds one feature, the control
    "s128": _ragged(28, 16, FOUR, 7004),    # two full slots
    "s129": _ragged(32, 1, FOUR, 7005),     # slot 2 holds one feature
    "s192": _ragged(44, 16, FOUR, 7120),    # three full slots
    "s193": _ragged(48, 1, FOUR, 7100),     # slot 3 holds one feature
    "s256": _ragged(60, 16, FOUR, 7521),    # four full slots
    "s257": _ragged(64, 1, FOUR, 7100),     # slot 4 holds one feature
}
NO_GOLDEN = ["s192", "s193", "s256", "s257"]     # their files would be the largest of tests/golden: data from the seed
EDGE = {
    # s63's data at the alpha where a gap decision is a real tie: status 2 by the gap margin alone
    "tie63": _ragged(31, 1, TWO, 7001, alpha=1e-2),
    # observation 1 identically zero: features 1 and 4 and targets 1 and 4 are zero (yy == 0, tol == 0)
    "zeroobs": _ragged(3, 1, TWO, 7011, alpha=1e-2, zero_obs=(1,)),
    # zero features on lanes 31 and 63 of slot 0, and slot 1's only feature (the control) zero
    "zeroedge": dict(_ragged(32, 1, TWO, 7012, zero_obs=(31,)), hold=(0, 0.0)),
    # a control that lost many digits to the centring but is still fitted: centred / raw = 4.1e-8, 2.7 x 2^-26 ...
    "near": _ragged(3, 2, TWO, 7013, alpha=1e-6, jitter=(1, 0.75, 2e-4)),
    # ... and one 2.3 times past the line (6.5e-9): status 1
    "past": _ragged(3, 2, TWO, 7013, alpha=1e-6, jitter=(1, 0.75, 8e-5)),
}
CASES.update(SWEEP)
CASES.update(EDGE)
FITTED = [n for n in CASES if n not in ("const", "past")]               # status 0 or 2: coefficients come back
# (case, alpha index) whose smallest gap margin lies within sysid.lasso_fit.TIE: status 2, on the host and the device
TIES = {("tie63", 0)}
# max|coef - reference| / max|reference| of lasso_fit_host against the reference's train(), the largest over the
# case's alphas, as gen_golden_lassofit.py printed it when the goldens were made (also stored in them as host_err);
# for the cases of NO_GOLDEN against sklearn's Lasso on the same design, as tests/test_lasso_fit_host.py prints it
HOST_ERR = {"n13": 3.4e-12, "dup": 6.3e-14, "n74": 6.8e-14, "big": 7.0e-14, "zero": 1.4e-14,
            "s15": 4.4e-15, "s63": 2.2e-14, "s64": 1.7e-14, "s65": 1.6e-14, "s128": 8.2e-14, "s129": 3.2e-14,
            "s192": 2.7e-13, "s193": 9.5e-14, "s256": 4.0e-13, "s257": 8.4e-14,
            "tie63": 3.8e-14, "zeroobs": 1.1e-14, "zeroedge": 1.8e-14, "near": 3.8e-8}


def alter(c, obs, ctrls):
    """Applies a case's changes to its concatenated data, in place."""
    for j in c.get("zero_obs", ()):
        obs[:, j] = 0.0
    if c.get("jitter") is not None:
        j, base, scale = c["jitter"]
        ctrls[:, j] = base * (1.0 + scale * np.random.default_rng(c["seed"] + 1).standard_normal(len(ctrls)))
    if c["hold"] is not None:
        ctrls[:, c["hold"][0]] = c["hold"][1]


def generate(name):
    """(traj_len, obs, ctrls) of a case from its seed (the goldens' dynamics)."""
    c = CASES[name]
    tr = make_trajs(system(c["no"], c["nu"]), c["lengths"], c["seed"])
    lens = np.array([len(t) for t in tr], dtype=np.int32)
    obs, ctrls = np.concatenate([t.obs for t in tr]), np.concatenate([t.ctrls for t in tr])
    alter(c, obs, ctrls)
    return lens, obs, ctrls


def gold(name):
    return np.load(os.path.join(GOLD, "lassofit_%s.npz" % name))


@functools.lru_cache(maxsize=None)
def _data(name):
    if name in NO_GOLDEN:
        out = generate(name)
    else:
        g = gold(name)
        out = g["traj_len"], g["obs"], g["ctrls"]
    for a in out:
        a.setflags(write=False)
    return out


def data(name):
    """(traj_len, obs, ctrls) of a case (read-only: shared by the tests)."""
    return _data(name)


def without_lone_rows(lens, obs, ctrls, after=0):
    """The data without the length-1 trajectories that start at data row >= after."""
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    drop = (np.asarray(lens) == 1) & (start >= after)
    rows = np.ones(len(obs), dtype=bool)
    rows[start[drop]] = False
    return np.asarray(lens)[~drop].copy(), obs[rows].copy(), ctrls[rows].copy()


def zero_columns(name):
    """(features, targets) that are identically zero in a case's design: the lifts of its zeroed observations, and
    a control held at 0."""
    c = CASES[name]
    nb, no = len(basis(name)[0]), c["no"]
    zt = sorted(b * no + j for b in range(nb) for j in c.get("zero_obs", ()))
    held = [nb * no + c["hold"][0]] if c["hold"] is not None and c["hold"][1] == 0.0 else []
    return np.array(zt + held, dtype=np.int64), np.array(zt, dtype=np.int64)


def trajs(name):
    c = CASES[name]
    s = system(c["no"], c["nu"])
    lens, obs, ctrls = data(name)
    out, r = [], 0
    for n in lens:
        out.append(Trajectory(s, int(n), obs[r:r + n].copy(), ctrls[r:r + n].copy()))
        r += int(n)
    return s, out


def new_model(s, name, alpha, method="lasso"):
    return Koopman(s, method=method, lasso_alpha=alpha, **CASES[name]["koopman"])


def basis(name):
    c = CASES[name]
    if "basis" in c:
        return c["basis"]
    return new_model(system(c["no"], c["nu"]), name, 1.0).device_lift()


@functools.lru_cache(maxsize=None)
def host(name):
    """lasso_fit_host on a case: (coeffs, status, margins, sweeps, per-target sweeps), computed once."""
    lens, obs, ctrls = data(name)
    return LS.lasso_fit_host(lens, obs, ctrls, [basis(name)], [(0, a) for a in CASES[name]["alphas"]],
                             per_target=True)


def reference(name, k):
    """([A | B], n_iter_ per target) of the reference for the case's k-th alpha; for the cases of NO_GOLDEN
    lasso_fit_host's (which tests/test_lasso_fit_host.py holds to sklearn's Lasso on those cases)."""
    if name in NO_GOLDEN:
        h = host(name)
        return h[0][k], h[4][k]
    g = gold(name)
    return np.hstack([g["A_%d" % k], g["B_%d" % k]]), g["n_iter_%d" % k]


def tolerance(name):
    """What the device may differ from the reference by: 100 x the case's recorded restatement error."""
    return 100.0 * HOST_ERR[name]


def rel_err(a, ref):
    return float(np.max(np.abs(np.asarray(a) - ref)) / max(np.max(np.abs(ref)), 1e-300))
