"""Shared by the stable-fit tests: the cases of tests/golden/gen_golden_stablefit.py (the reference's own
stabilize_discrete on each), the models that go with them, and the inputs of the tests that need no golden."""
import os

import numpy as np

from autompc_amd import Koopman, Trajectory

from linfit_cases import system

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# name -> observations, controls, trajectory lengths, data seed, spectral radius of the linear part of the dynamics,
# start amplitude, Koopman arguments (gain: the scale of the control matrix, 0.1 when absent).  Smallest first.
CASES = {
    # the smallest: identity basis, 33 design rows, one partial tile everywhere
    "n2": dict(no=2, nu=1, lengths=[12] * 3, seed=401, rho=1.06, amp=0.5, koopman=dict()),
    # x, x^2, sin x, cos x of 3 observations: n = 12, no multiple of 16
    "n12": dict(no=3, nu=1, lengths=[40] * 6, seed=402, rho=1.015, amp=0.4,
                koopman=dict(strict_reference=False, poly_basis=True, poly_degree=2, trig_basis=True, trig_freq=1)),
    # 17 observations x 3 basis functions, 6 controls, 1980 design rows: several row splits of the Gram pass
    "n51": dict(no=17, nu=6, lengths=[100] * 20, seed=403, rho=1.004, amp=0.5,
                koopman=dict(strict_reference=False, trig_basis=True, trig_freq=1)),
    # the size limit: 4 observations x 16 basis functions (x, x^2, sin / cos of x .. 7 x)
    "n64": dict(no=4, nu=2, lengths=[12] * 60, seed=404, rho=1.01, amp=2.0, gain=0.05,
                koopman=dict(strict_reference=False, poly_basis=True, poly_degree=2, trig_basis=True, trig_freq=7)),
    # the least-squares A is already stable: the clip at 1 stays idle
    "inactive": dict(no=3, nu=1, lengths=[40] * 4, seed=415, rho=0.9, amp=1.0,
                     koopman=dict(strict_reference=False, poly_basis=True, poly_degree=2)),
    # the strict-reference basis of poly_degree 3: x, x^3 twice -> a singular Gram -> status 1 -> the host route.  (The
    # reference's own result on a singular design hangs on its pseudo-inverse cutoff and its unsymmetric ``eig``: it is
    # recorded, and compared with nothing.)
    "dup": dict(no=2, nu=1, lengths=[30] * 5, seed=406, rho=1.01, amp=0.4,
                koopman=dict(poly_basis=True, poly_degree=3)),
}
FITTED = [n for n in CASES if n != "dup"]

# The size sweep: identity basis on n observations (n lifted states) and nu controls, just enough trajectories of 12
# rows for a well-posed design (from n = 45 on more than 512 data rows: two row splits).  Sizes: the smallest and the
# largest, both parities around every multiple of 16 (the eigensolver pads odd n to n + 1; at n = 63 the pad row is the
# last LDS row), and with nu = 1 / 16 every layout where n + nu is a multiple of 16, so that Y starts on a tile edge
# (15 + 1, 16 + 16, 48 + 16, 64 + 16: the last is 9 x 9 tiles).  The seed is 1000 + 100 nu + n unless SWEEP_SEEDS
# names another: n = 2 ties at the rule's seeds (a case whose reference run came within TIE of a decision takes the
# next seed that does not).  n = 1 always ties and is kept as that (status 2: with the clip at 1 active A = S^-1 U B S
# = +-1 whatever the trial makes of S, so the error repeats, exactly or to the last bits of a converged Bcon).
SWEEP_N = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63, 64)
SWEEP_NU = (1, 16)
SWEEP_SEEDS = {(2, 1): 5001, (2, 16): 5001}


def _sweep_case(n, nu):
    k = max(3, (8 * (n + nu) + 20) // 11 + 1)
    return dict(no=n, nu=nu, lengths=[12] * k, seed=SWEEP_SEEDS.get((n, nu), 1000 + 100 * nu + n), rho=1.02, amp=0.5,
                koopman=dict())


SWEEP = {"sweep_n%d_u%d" % (n, nu): _sweep_case(n, nu) for nu in SWEEP_NU for n in SWEEP_N}
# ragged rows: data row 511, the last of the first row split, is a trajectory's last row; row 512, the first of the
# second split, is a trajectory of length 1 (no design row); three more length-1 trajectories lie about
# (seed: 6105 makes the reference's own inv(S) raise "Singular matrix" in a line search; 6106 is the next)
SWEEP["sweep_ragged"] = dict(no=5, nu=2, lengths=[1, 2, 509, 1, 1, 30, 2, 1, 40], seed=6106, rho=1.01, amp=0.5,
                             koopman=dict())
SWEEP_TIED = [n for n in SWEEP if SWEEP[n]["no"] == 1]      # status 2: no reference comparison
SWEEP_FITTED = [n for n in SWEEP if n not in SWEEP_TIED]

# one declined basis inside the kernel: with observation 2 zero on every row that is not a trajectory's first, every
# target of that state is zero, row 2 of the least-squares W0 is exactly zero and the first polar factor declines
DECLINED = dict(no=4, nu=2, lengths=[12] * 8, seed=77, rho=1.02, amp=0.5)
# three bases of one data set at the control limit: x; x, sin x; x, sin x, cos x -> n = 21, 42, 63 in one launch
MIXED = dict(no=21, nu=16, lengths=[12] * 70, seed=6021, rho=1.01, amp=0.5)
MIXED_BASES = [([0], [1.0]), ([0, 2], [1.0, 1.0]), ([0, 2, 3], [1.0, 1.0, 1.0])]


def case(name):
    return CASES[name] if name in CASES else SWEEP[name]


def make_data(name):
    """(traj_len, obs, ctrls) of a case (its name, or a dict like a case's): a slightly unstable rotation plus a small
    sine term, random controls and measurement noise; short trajectories keep it bounded."""
    c = case(name) if isinstance(name, str) else name
    no, nu = c["no"], c["nu"]
    rng = np.random.default_rng(c["seed"])
    K = rng.normal(size=(no, no))
    w, V = np.linalg.eig(0.3 * (K - K.T) / np.sqrt(no))         # a rotation generator
    M = c["rho"] * np.real((V * np.exp(w)) @ np.linalg.inv(V))
    Gm = rng.normal(scale=c.get("gain", 0.1), size=(no, nu))
    obs, ctrls = [], []
    for T in c["lengths"]:
        x = rng.uniform(-c["amp"], c["amp"], size=no)
        for _ in range(T):
            u = rng.uniform(-1.0, 1.0, size=nu)
            obs.append(x + rng.normal(scale=0.01, size=no))
            ctrls.append(u)
            x = M @ x + 0.05 * np.sin(2.0 * x[::-1]) + Gm @ u
    return np.array(c["lengths"], dtype=np.int32), np.array(obs), np.array(ctrls)


def gold(name):
    return np.load(os.path.join(GOLD, "stablefit_%s.npz" % name))


def data(name):
    g = gold(name)
    return g["traj_len"], g["obs"], g["ctrls"]


def trajs(name):
    c = case(name)
    s = system(c["no"], c["nu"])
    lens, obs, ctrls = data(name)
    out, r = [], 0
    for n in lens:
        out.append(Trajectory(s, int(n), obs[r:r + n].copy(), ctrls[r:r + n].copy()))
        r += int(n)
    return s, out


def new_model(s, name, method="stable"):
    return Koopman(s, method=method, **case(name)["koopman"])


def basis(name):
    return new_model(system(case(name)["no"], case(name)["nu"]), name).device_lift()


def reference(name):
    """[A | B] of the reference."""
    g = gold(name)
    return np.hstack([g["A"], g["B"]])


def tolerance(name):
    """What the Gram form (host or device) may differ from the reference by: 100 x the larger of the restatement's
    recorded error and the case's recorded round-off response."""
    g = gold(name)
    return 100.0 * max(float(g["host_err"]), float(g["roundoff_response"]))


def rel_err(a, ref):
    return float(np.max(np.abs(np.asarray(a) - ref)) / max(np.max(np.abs(ref)), 1e-300))


def declined_data():
    """(traj_len, obs, ctrls) of DECLINED."""
    lens, obs, ctrls = make_data(DECLINED)
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    later = np.ones(len(obs), dtype=bool)
    later[first] = False
    obs[later, 2] = 0.0
    return lens, obs, ctrls


def two_valued_data():
    """(traj_len, obs, ctrls) of DECLINED's data with observation 2 replaced by 0 / 1 (above its median or not): the
    identity basis fits it (host form: status 0, 29 iterations, margin 1e-6), and x^2 of that observation equals it,
    so a basis with x and x^2 has a singular Gram.  (A lifted column that is zero while the identity basis stays
    fitted does not exist: f(x) = x^2, sin or a power is zero only where x is, and an all-zero observation, or one
    whose successors are all zero, declines the identity basis as well.)"""
    lens, obs, ctrls = make_data(DECLINED)
    obs[:, 2] = (obs[:, 2] > np.median(obs[:, 2])).astype(np.float64)
    return lens, obs, ctrls


def without_lone_rows(lens, obs, ctrls, split=512):
    """The data set without its length-1 trajectories (they have no design row), except that where a removal would
    pull a later trajectory across a row-split boundary (every `split` data rows: linear_fit.SPLIT_ROWS) one removed
    lone row per missing row is put back as padding in front of it.  Every remaining row keeps its split and its
    order; its position within the split moves."""
    lens = np.asarray(lens)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    lone = [int(s) for s, n in zip(starts, lens) if n == 1]
    out_lens, rows = [], []
    for s, n in zip(starts, lens):
        if n == 1:
            continue
        while len(rows) // split < s // split:
            out_lens.append(1)
            rows.append(lone[0])
        out_lens.append(int(n))
        rows.extend(range(s, s + n))
    rows = np.array(rows)
    kept = np.repeat(np.array(out_lens) > 1, out_lens)
    assert np.array_equal(rows[kept] // split, np.nonzero(kept)[0] // split) and np.all(np.diff(rows[kept]) > 0)
    return np.array(out_lens, dtype=np.int32), obs[rows].copy(), ctrls[rows].copy()


def perturbation(seed):
    """perturb(G, Q, yy) for stable_fit_host: every Gram entry times 1 + 2^-52 z, z seeded uniform in [-1, 1]
    (symmetrically in G): one rounding.  The change of the fit under it is a case's roundoff_response."""
    rng = np.random.default_rng(seed)

    def perturb(Gm, Q, yy):
        Z = rng.uniform(-1.0, 1.0, size=Gm.shape)
        Z = np.triu(Z) + np.triu(Z, 1).T
        return (Gm * (1.0 + 2.0 ** -52 * Z), Q * (1.0 + 2.0 ** -52 * rng.uniform(-1.0, 1.0, size=Q.shape)),
                yy * (1.0 + 2.0 ** -52 * rng.uniform(-1.0, 1.0, size=yy.shape)))
    return perturb


def residual(coeffs, lens, obs, ctrls, b):
    """|Y - A Xs - B Xu|_F of [A | B] = coeffs over the design rows of basis b, in extended precision."""
    from autompc_amd.sysid.stable_fit import koopman_rows
    Xs, Xu, Y = (np.asarray(a, dtype=np.longdouble) for a in koopman_rows(lens, obs, ctrls, b))
    n = Xs.shape[0]
    W = np.asarray(coeffs, dtype=np.longdouble)
    E = Y - W[:, :n] @ Xs - W[:, n:] @ Xu
    return float(np.sqrt(np.sum(E * E)))
