"""Shared by the LQR edge tests (test_gpu_lqr_edges.py, test_lqr_host.py) and their generator
(golden/gen_golden_lqr_edges.py): seeded problems at the gain kernel's tile edges and limits with diagonal,
non-symmetric and pivoting costs; a numpy model of ``lqr_gains_kernel``'s arithmetic; the reference's recursion in any
float type; the closed loop of ``simulate()`` + ``FiniteHorizonLQR.run`` restated in any float type.

Inputs come from ``default_rng(seed)`` by elementwise arithmetic alone (no LAPACK), and the fixture keeps an exact
checksum of each, so a random stream that drifted between machines fails as that."""
import functools
import math
import os

import numpy as np

RHO, B_SCALE = 0.8, 0.3
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lqr_edges.npz")

# (n, nu, no, horizon, kind).  Shapes: n = 1; no == n; the 16-deep k slice (16 / 17); both sides of the 64-wide tile
# at 64, 128, 192 and 256; m = n + nu on a tile multiple (60 + 4, 240 + 16) and one past it (60 + 5); nu up to 16;
# the plan maximum.  Horizon 1000 once, at n = 65; three steps or fewer from n = 192 up.  Kinds: every kind at
# n <= 64, at a tile edge and at n >= 240 with nu = 16 (n = 256 / nu = 16 / no = 17 carries two).  The last two rows
# exist for the closed-loop plans (rule 0 needs n == no at that plan's nu).
_SHAPES = [
    (1, 1, 1, 7, "diag"), (16, 1, 16, 7, "asym"), (17, 2, 5, 7, "pivot"), (60, 4, 6, 20, "pivot_asym"),
    (60, 5, 6, 20, "diag"), (63, 16, 8, 20, "asym"), (64, 16, 64, 20, "pivot"), (65, 7, 5, 1000, "asym"),
    (127, 15, 9, 5, "pivot_asym"), (128, 16, 17, 5, "diag"), (129, 3, 17, 5, "pivot"), (192, 16, 6, 3, "asym"),
    (193, 1, 6, 3, "diag"), (240, 16, 17, 2, "pivot_asym"), (255, 15, 17, 2, "asym"), (256, 16, 17, 2, "diag"),
    (256, 16, 17, 2, "pivot"), (256, 16, 256, 1, "asym"), (256, 1, 1, 2, "diag"),
    (17, 16, 17, 5, "diag"), (5, 7, 5, 5, "pivot"),
]
CASES = {"n%d_u%d_o%d_%s" % (n, nu, no, kind): dict(n=n, nu=nu, no=no, horizon=hz, kind=kind, seed=7000 + i)
         for i, (n, nu, no, hz, kind) in enumerate(_SHAPES)}
# at their first seed these two diagonal-R cases exchange rows in some solve (no = 6 of n = 60 / 192 states leaves
# B'PB of rank 6, as large off the diagonal as on it): the next seed in steps of 100 at which none does
CASES["n60_u5_o6_diag"]["seed"] = 7204
CASES["n192_u16_o6_asym"]["seed"] = 7311
KINDS = ("diag", "asym", "pivot", "pivot_asym")


def pivoting(name):
    return CASES[name]["kind"].startswith("pivot")


def plan_groups():
    """Case names by (no, nu): the cases that can share one plan."""
    out = {}
    for name, c in CASES.items():
        out.setdefault((c["no"], c["nu"]), []).append(name)
    return out


def costs(kind, no, nu, rng):
    """Q, R, F of a cost kind.  diag: random diagonals over two decades.  asym: Q and F get a strictly upper
    triangle.  pivot: R = D^1/2 C D^1/2 with D = 2^i and C's off-diagonals near 0.9 (symmetric positive definite; in
    column 0 the last row, 0.9 sqrt(2^(nu-1)), beats the diagonal 1), Q and F a hundredth so that R dominates B'PB.
    pivot_asym: that R plus a strictly upper triangle."""
    Q = np.diag(10 ** rng.uniform(-1, 1, no))
    R = np.diag(10 ** rng.uniform(-1, 1, nu))
    F = np.diag(10 ** rng.uniform(-1, 1, no))
    if kind == "asym":
        Q = Q + 0.3 * np.triu(rng.normal(size=(no, no)), 1)
        F = F + 0.3 * np.triu(rng.normal(size=(no, no)), 1)
    if kind.startswith("pivot"):
        rd = np.sqrt(2.0 ** np.arange(nu))
        u = np.triu(rng.uniform(-1, 1, size=(nu, nu)), 1)
        C = 0.9 + 0.005 * (u + u.T)
        np.fill_diagonal(C, 1.0)
        R = rd[:, None] * C * rd[None, :]
        Q, F = 0.01 * Q, 0.01 * F
        if kind == "pivot_asym":
            R = R + 0.05 * rd[:, None] * np.triu(rng.normal(size=(nu, nu)), 1) * rd[None, :]
    return Q, R, F


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(A, B, Q, R, F) of a case: A = RHO normal / sqrt(n), B = B_SCALE normal."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    n, nu = c["n"], c["nu"]
    A = RHO * rng.normal(size=(n, n)) / np.sqrt(n)
    B = B_SCALE * rng.normal(size=(n, nu))
    out = (A, B) + costs(c["kind"], c["no"], nu, rng)
    for a in out:
        a.setflags(write=False)
    return out


def checksum(arrays):
    """[[sum, sum of squares]] of each array, summed exactly (fsum), so equal inputs give equal bits anywhere."""
    return np.array([[math.fsum(a.ravel()), math.fsum((a * a).ravel())] for a in arrays])


def pad(X, n, dtype=np.float64):
    out = np.zeros((n, n), dtype=dtype)
    out[:X.shape[0], :X.shape[1]] = X
    return out


def gauss_jordan(S, Y):
    """The kernel's solve of S X = Y: Gauss-Jordan on [S | Y] with partial pivoting, the first row of the largest
    magnitude taken.  Any float type.  Returns (X, row exchanges), X None on an exact zero or non-finite pivot."""
    aug = np.hstack([S, Y])
    nu = S.shape[0]
    exchanges = 0
    for c in range(nu):
        p, best = c, abs(aug[c, c])
        for r in range(c + 1, nu):
            if abs(aug[r, c]) > best:
                p, best = r, abs(aug[r, c])
        if not best > 0 or not np.isfinite(best):
            return None, exchanges
        if p != c:
            aug[[c, p]] = aug[[p, c]]
            exchanges += 1
        aug[c, c + 1:] /= aug[c, c]
        f = aug[:, c].copy()
        f[c] = 0
        aug[:, c + 1:] -= f[:, None] * aug[c, c + 1:][None, :]
    return aug[:, nu:], exchanges


def kernel_model(A, B, Q, R, F, horizon):
    """lqr_gains_kernel's arithmetic in numpy f64 (csrc/lqr_kernels.hpp), up to the order of the sums:
    M = P [A | B], G = [A | B]' M, X = (R + G_BB)^-1 G_BA, P <- (G_AA - G_AB X) + Q, horizon + 1 times from P = F,
    then K = -X.  Returns (K, status, row exchanges of every solve)."""
    n, nu = B.shape
    AB = np.hstack([A, B])
    P, Qp = pad(F, n), pad(Q, n)
    counts = []
    for it in range(horizon + 2):
        G = AB.T @ (P @ AB)
        X, ex = gauss_jordan(R + G[n:, n:], G[n:, :n])
        counts.append(ex)
        if X is None or not np.all(np.isfinite(X)):
            return np.full((nu, n), np.nan), 1, counts
        if it == horizon + 1:
            return -X, 0, counts
        P = (G[:n, :n] - G[:n, n:] @ X) + Qp


def riccati(A, B, Q, R, F, horizon, dtype=np.longdouble):
    """K of the reference's _finite_horz_dt_lqr(A, B, Q, R, 0, F, horizon) (lqr.py:15-47) in its own association
    order, in `dtype`, the inverse by gauss_jordan (numpy's LAPACK has no long double)."""
    n, nu = B.shape
    A, B, R = (np.asarray(x, dtype=dtype) for x in (A, B, R))
    Qp, P = pad(Q, n, dtype), pad(F, n, dtype)
    eye = np.eye(nu, dtype=dtype)

    def inv(S):
        X, _ = gauss_jordan(S, eye)
        if X is None:
            raise np.linalg.LinAlgError("Singular matrix")
        return X
    for _ in range(horizon + 1):
        AtP, BtP = A.T @ P, B.T @ P
        P = AtP @ A - (AtP @ B) @ inv(R + BtP @ B) @ (BtP @ A) + Qp
    BtP = B.T @ P
    return -inv(R + BtP @ B) @ B.T @ P @ A


def rel_err(a, ref):
    """max|d| / max|ref|, in ref's float type."""
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(a, dtype=ref.dtype) - ref)) / np.max(np.abs(ref)))


def tolerance(host_err):
    """The project's rule for a device result against an extended-precision one: a hundred times
    what the host's f64 restatement loses, and never below 1e-13."""
    return max(100.0 * float(host_err), 1e-13)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLD))


# ---- closed loop ---------------------------------------------------------------------------------------------------
# One plan per (no, nu): the plan fixes both, and rule 0 needs n == no.  problems: (case, rule).  The surrogate is a
# linear model of snx > no states drawn like the cases' A and B.  lo / hi differ per control: control 0 is free, 1 is
# bounded above only, 2 below only (where the plan has that many), the rest on both sides, tight enough to bind.
T_LOOP = 20
LOOPS = {
    "o17_u16": dict(no=17, nu=16, snx=20, seed=7101,
                    problems=[("n256_u16_o17_diag", 1), ("n17_u16_o17_diag", 0), ("n128_u16_o17_diag", 1)]),
    "o1_u1": dict(no=1, nu=1, snx=3, seed=7102, problems=[("n1_u1_o1_diag", 0), ("n256_u1_o1_diag", 1)]),
    "o5_u7": dict(no=5, nu=7, snx=8, seed=7103, problems=[("n65_u7_o5_asym", 1), ("n5_u7_o5_pivot", 0)]),
}


def loop_bounds(nu):
    i = np.arange(nu, dtype=np.float64)
    lo, hi = -(0.02 + 0.01 * i), 0.03 + 0.005 * i
    lo[0], hi[0] = -np.inf, np.inf
    if nu > 1:
        lo[1] = -np.inf
    if nu > 2:
        hi[2] = np.inf
    return lo, hi


@functools.lru_cache(maxsize=None)
def make_loop(name):
    """dict(As, Bs, lo, hi, goal [B][no], sim0 [B][snx], s0: list of [n_i]) of a closed-loop plan."""
    L = LOOPS[name]
    no, nu, snx = L["no"], L["nu"], L["snx"]
    rng = np.random.default_rng(L["seed"])
    As = RHO * rng.normal(size=(snx, snx)) / np.sqrt(snx)
    Bs = B_SCALE * rng.normal(size=(snx, nu))
    B = len(L["problems"])
    goal = rng.uniform(-0.3, 0.3, size=(B, no))
    sim0 = rng.uniform(-0.5, 0.5, size=(B, snx))
    s0 = []
    for i, (case, rule) in enumerate(L["problems"]):
        s = rng.uniform(-0.5, 0.5, size=CASES[case]["n"])
        s0.append(sim0[i, :no].copy() if rule == 0 else s)
    lo, hi = loop_bounds(nu)
    return dict(As=As, Bs=Bs, lo=lo, hi=hi, goal=goal, sim0=sim0, s0=s0)


def closed_loop(A, B, K, rule, no, goal, s0, sim0, As, Bs, lo, hi, T, dtype):
    """simulate() (utils/simulation.py:44-63) driving FiniteHorizonLQR.run (lqr.py:174-192) against the linear
    surrogate sim' = As sim + Bs u, in `dtype`.  rule 0: the model state is the observation; rule 1: A s + B u_prev
    with the observation slot overwritten (arx.py:94-99), the first step included.  Returns (obs [T+1][no],
    ctrls [T+1][nu], the last row zero)."""
    A, B, K, As, Bs, lo, hi = (np.asarray(x, dtype=dtype) for x in (A, B, K, As, Bs, lo, hi))
    n, nu = B.shape
    state0 = np.zeros(n, dtype=dtype)
    state0[:no] = goal
    s, sim, u = np.asarray(s0, dtype=dtype), np.asarray(sim0, dtype=dtype), np.zeros(nu, dtype=dtype)
    obs, ctrls = np.zeros((T + 1, no), dtype=dtype), np.zeros((T + 1, nu), dtype=dtype)
    obs[0] = sim[:no]
    for step in range(T):
        if rule == 0:
            s = sim[:no].copy()
        else:
            s = A @ s + B @ u
            s[:no] = sim[:no]
        u = K @ (s - state0)
        u = np.minimum(u, hi)
        u = np.maximum(u, lo)
        sim = As @ sim + Bs @ u
        obs[step + 1], ctrls[step] = sim[:no], u
    return obs, ctrls


def clipping(ctrls, lo, hi):
    """(some control on its upper bound at some step, some on its lower, some never clipped) of a trajectory."""
    c = np.asarray(ctrls[:-1], dtype=np.float64)
    up, low = np.any(c == hi, axis=0), np.any(c == lo, axis=0)
    return bool(up.any()), bool(low.any()), bool(np.any(~up & ~low))
