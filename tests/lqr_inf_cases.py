"""Shared by the infinite-horizon LQR tests (test_gpu_lqr_inf.py, test_gpu_lqr_inf_eval.py): the fixtures of
golden/gen_golden_lqr_inf.py and their models; the reference's fixed-point iteration (_inf_horz_dt_lqr, lqr.py:22-33)
in any float type; seeded problems at the gain kernel's block and tile edges.

Inputs come from ``default_rng(seed)`` by elementwise arithmetic alone, as in lqr_edge_cases.py."""
import functools
import os

import numpy as np

import lqr_edge_cases as E

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = [("arx2", 4, 1), ("koop_mlp", 4, 1), ("arx4_mlp", 17, 6), ("arx10_wide", 17, 6)]
MARGIN = 1e-6             # every dP of a counted iteration stays this far (relative) from its threshold


def gold(name):
    return np.load(os.path.join(GOLD, "lqrinf_%s.npz" % name))


def system(no, nu):
    from autompc_amd import System
    return System(["x%d" % i for i in range(no)], ["u%d" % i for i in range(nu)], dt=0.05)


def model_of(name, g, no, nu):
    from autompc_amd import ARX, Koopman
    s = system(no, nu)
    if name == "koop_mlp":
        m = Koopman(s, method="lstsq", poly_basis=True, poly_degree=int(g["poly_degree"]))
        m.set_parameters({"A": g["A"], "B": g["B"]})
    else:
        m = ARX(s, history=int(g["history"]))
        m.set_parameters({"coeffs": g["coeffs"]})
    return s, m


def seeded_mlp(sys_, hidden, activation, seed):
    """The surrogate of a fixture (gen_golden.ref_mlp: oracle.mlp.random_params + gen_golden.normalisers)."""
    from autompc_amd import MLP
    from oracle import mlp as omlp
    no, nu = sys_.obs_dim, sys_.ctrl_dim
    p = omlp.random_params(no, nu, hidden, activation, seed=seed)
    rng = np.random.default_rng(seed + 7919)
    p["xu_means"], p["xu_std"] = rng.normal(scale=0.3, size=no + nu), rng.uniform(0.5, 2.0, size=no + nu)
    p["dy_means"], p["dy_std"] = rng.normal(scale=0.02, size=no), rng.uniform(0.05, 0.2, size=no)
    m = MLP(sys_, n_hidden_layers=len(hidden), hidden_size=hidden[0], nonlintype=activation)
    m.weights, m.biases = p["weights"], p["biases"]
    m.xu_means, m.xu_std, m.dy_means, m.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
    return m


def surrogate_of(name, g, s, m):
    if "sur_seed" not in g:
        return m
    act = "relu" if name == "koop_mlp" else "tanh"
    return seeded_mlp(s, [int(v) for v in g["sur_hidden"]], act, int(g["sur_seed"]))


def riccati_inf(A, B, Q, R, threshold, max_iter=100000, dtype=np.longdouble):
    """(K, iters, dP) of the reference's _inf_horz_dt_lqr(A, B, Qp, R, 0, threshold) in its own association order, in
    `dtype`, the inverse by lqr_edge_cases.gauss_jordan.  dP: max|P_new - P_old| after every step.  K is None when P
    still moves after max_iter steps."""
    n, nu = B.shape
    A, B, R = (np.asarray(x, dtype=dtype) for x in (A, B, R))
    Qp = E.pad(Q, n, dtype)
    eye = np.eye(nu, dtype=dtype)

    def inv(S):
        X, _ = E.gauss_jordan(S, eye)
        if X is None:
            raise np.linalg.LinAlgError("Singular matrix")
        return X

    def step(P):
        AtP, BtP = A.T @ P, B.T @ P
        return AtP @ A - (AtP @ B) @ inv(R + BtP @ B) @ (BtP @ A) + Qp
    P1, P2 = Qp, step(Qp)
    dP = [np.abs(P1 - P2).max()]
    while dP[-1] > threshold:
        if len(dP) >= max_iter:
            return None, len(dP), np.array(dP, dtype=np.float64)
        P1, P2 = P2, step(P2)
        dP.append(np.abs(P1 - P2).max())
    BtP = B.T @ P2
    return -inv(R + BtP @ B) @ B.T @ P2 @ A, len(dP), np.array(dP, dtype=np.float64)


def margin_ok(dP, threshold, converged=True):
    """No dP of the sequence is within MARGIN (relative) of the threshold, so one rounding cannot change the count."""
    dP = np.asarray(dP, dtype=np.float64)
    head = dP[:-1] if converged else dP
    ok = bool(np.all(head > threshold * (1 + MARGIN)))
    return ok and (not converged or bool(dP[-1] < threshold * (1 - MARGIN)))


# ---- shape edges: (n, nu, no, threshold, seed) ----------------------------------------------------------------------
# n on both sides of the update's 8 x 8 blocks (7, 8, 9) and of the products' 64-wide tile (63, 64, 65), n = 1, and
# 256 (1024 blocks for four waves); nu from 1 to 16; no < n and no == n.  The 256-state problem stops at a coarser
# threshold (7 steps for 12): its long-double iteration is the slowest thing here, and the count is as exact there.
EDGES = {
    "n1": (1, 1, 1, 1e-3, 8100), "n7": (7, 2, 7, 1e-3, 8101), "n8": (8, 3, 5, 1e-3, 8102),
    "n9": (9, 16, 9, 1e-3, 8103), "n63": (63, 5, 6, 1e-3, 8104), "n64": (64, 16, 64, 1e-3, 8105),
    "n65": (65, 7, 5, 1e-3, 8106), "n256": (256, 16, 17, 1e-2, 8107),
}


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(A, B, Q, R) of an edge case: A = 0.8 normal / sqrt(n), B = 0.3 normal, diagonal Q and R over two decades."""
    n, nu, no, _, seed = EDGES[name]
    rng = np.random.default_rng(seed)
    A = E.RHO * rng.normal(size=(n, n)) / np.sqrt(n)
    B = E.B_SCALE * rng.normal(size=(n, nu))
    Q, R, _ = E.costs("diag", no, nu, rng)
    for a in (A, B, Q, R):
        a.setflags(write=False)
    return A, B, Q, R


@functools.lru_cache(maxsize=None)
def edge_expected(name):
    """(K long double, iters, dP) of an edge case, computed once."""
    return riccati_inf(*edge_case(name), EDGES[name][3])


def slow_mode_case(s, n=65, nu=2, seed=8200):
    """Diagonal A, every mode 0.3 but one slow one (0.97) at index s; B = 1e-3 normal; Q = R = I (no == n): the entry
    of P that decides when the iteration stops is P[s][s] alone."""
    rng = np.random.default_rng(seed)
    a = np.full(n, 0.3)
    a[s] = 0.97
    return np.diag(a), 1e-3 * rng.normal(size=(n, nu)), np.eye(n), np.eye(nu)


def bias_system(bias=0.05, seed=11):
    """4 observed states plus a constant state (A's last row e_n, as ARX's) that feeds them a bias: the constant
    state earns the same stage cost every step, so P's corner entry grows by a constant for ever."""
    rng = np.random.default_rng(seed)
    A = np.zeros((5, 5))
    A[:4, :4] = 0.8 * rng.normal(size=(4, 4)) / 2.0
    A[:4, 4] = bias
    A[4, 4] = 1.0
    B = np.zeros((5, 1))
    B[:4] = 0.3 * rng.normal(size=(4, 1))
    return A, B, np.eye(4), np.eye(1)
