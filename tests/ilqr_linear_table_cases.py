"""Shared by the tests of the iLQR plan that holds a table of linear models of mixed state dimension
(ampc_ilqr_plan_set_linear_models, csrc/ilqr_linear_table_kernels.hpp): three sets of synthetic models x' = A x + B u,
built as mppi_linear_table_cases.matrices builds them, and for every set ONE fixed list of problems -- model, horizon,
cost block, initial state -- under control bounds (-1, 1) and one plan horizon of 8.

  edges  3 observations / 2 controls  nx 3 (= obs_dim, rule 0), 14, 15, 16, 17: nx + nu crosses 16 (the Jacobian's
                                      padded width ldj 16 -> 32) while nxp stays 16, then both cross
  wide   3 / 2                        nx 62, 64, 65 (the staging boundary of ampc_set_linear), 126 (nx + nu = 128), 128
                                      (the limit); dense cost blocks
  nu6    5 / 6                        nx 5 (= obs_dim), 23, 70, 122 (nx + nu = 128)

Horizons are 1, 2, 5 and 8; every problem has a cost block of its own; model_index is non-monotonic; the LAST table
entry of every set is used by no problem; there are more problems (10) than slots (4, 2), so that slots refill with a
model of another size.  oracle_solves() is the oracle's iLQR on every problem's (A, B), once on the matrices and once on
matrices perturbed by 1e-12 relative: tests/test_ilqr_linear_table_host.py checks on the CPU that both runs take the
same decisions -- the precondition of comparing the device's decisions with the oracle's.  A problem that fails it is
replaced HERE, not excused in a test."""
import functools

import numpy as np

from helpers import make_system

PLAN_H = 8
DT = 0.05
LO, HI = -1.0, 1.0
MAX_ITER = 50
# (obs_dim, nu, state dimensions of the table, model / horizon of each problem, dense cost blocks, the range of the
# initial states -- wide enough for the bounds to bite); the last entry is a spare nobody uses
SETS = {
    "edges": dict(no=3, nu=2, nx=(3, 14, 15, 16, 17, 9), index=(4, 0, 3, 1, 2, 4, 0, 1, 3, 2),
                  hz=(8, 5, 1, 2, 8, 2, 8, 5, 5, 1), dense=False, x0=0.5),
    "wide": dict(no=3, nu=2, nx=(62, 64, 65, 126, 128, 40), index=(2, 4, 0, 3, 1, 4, 3, 0, 2, 1),
                 hz=(5, 8, 2, 8, 1, 2, 5, 8, 1, 5), dense=True, x0=2.0),
    "nu6": dict(no=5, nu=6, nx=(5, 23, 70, 122, 11), index=(2, 0, 3, 1, 3, 0, 2, 1, 3, 0),
                hz=(8, 2, 5, 1, 8, 5, 2, 8, 1, 8), dense=False, x0=2.0),
}


@functools.lru_cache(maxsize=None)
def matrices(name):
    """(system, [(A, B) ...]) of a set.  Read-only."""
    s = SETS[name]
    out = []
    for k, nx in enumerate(s["nx"]):
        rng = np.random.default_rng(2000 * len(name) + 10 * k + nx)
        A = 0.9 * np.linalg.qr(rng.normal(size=(nx, nx)))[0] + 0.02 * rng.normal(size=(nx, nx)) / np.sqrt(nx)
        assert np.max(np.abs(np.linalg.eigvals(A))) < 1.0
        B = rng.normal(scale=0.3, size=(nx, s["nu"]))
        A.setflags(write=False)
        B.setflags(write=False)
        out.append((A, B))
    return make_system(s["no"], s["nu"]), out


@functools.lru_cache(maxsize=None)
def problems(name):
    """The set's problems: model index [P], horizon [P], x0 (a list, each its model's state dimension) and a cost block
    per problem (Q, R, F [P][..][..], goal [P][no]).  Read-only: the tests share it."""
    s = SETS[name]
    no, nu = s["no"], s["nu"]
    rng = np.random.default_rng({"edges": 61, "wide": 62, "nu6": 63}[name])
    P = len(s["index"])

    def psd(n, lo, hi):
        if not s["dense"]:
            return np.diag(rng.uniform(lo, hi, n))
        W = rng.normal(size=(n, n))
        return W @ W.T / n * lo + np.diag(rng.uniform(lo, hi, n))
    d = dict(index=np.array(s["index"], dtype=np.int32), hz=np.array(s["hz"], dtype=np.int32),
             x0=[rng.uniform(-s["x0"], s["x0"], size=s["nx"][k]) for k in s["index"]],
             Q=np.stack([psd(no, 0.5, 2.0) for _ in range(P)]),
             R=np.stack([psd(nu, 0.05, 0.2) for _ in range(P)]),
             F=np.stack([psd(no, 0.5, 2.0) for _ in range(P)]),
             goal=rng.normal(scale=0.1, size=(P, no)))
    for v in d.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return d


class LinearModel:
    """x' = A x + B u for oracle.ilqr.ILQROracle."""

    def __init__(self, system, A, B):
        self.system, self.A, self.B = system, np.asarray(A), np.asarray(B)
        self.state_dim = self.A.shape[0]

    def pred(self, s, u):
        return self.A @ s + self.B @ u

    def pred_batch(self, s, u):
        return s @ self.A.T + u @ self.B.T

    def pred_diff(self, s, u):
        return self.A @ s + self.B @ u, self.A.copy(), self.B.copy()

    def pred_diff_batch(self, s, u):
        n = s.shape[0]
        return s @ self.A.T + u @ self.B.T, np.tile(self.A, (n, 1, 1)), np.tile(self.B, (n, 1, 1))


def oracle_solve(system, A, B, Q, R, F, goal, horizon, x0, max_iter=MAX_ITER):
    """The oracle's iLQR on one problem: dict(converged, iters, states, ctrls, Ks, ks, objective)."""
    from oracle.costs import QuadCostOracle
    from oracle.ilqr import ILQROracle
    nu = system.ctrl_dim
    orc = ILQROracle(LinearModel(system, A, B), QuadCostOracle(Q, R, F, goal), DT, int(horizon),
                     ubounds=(np.full(nu, LO), np.full(nu, HI)), max_iter=max_iter)
    conv, st, ct, Ks, ks = orc.solve(np.array(x0), np.zeros((int(horizon), nu)))
    return dict(converged=bool(conv), iters=int(orc.n_iter), states=st, ctrls=ct, Ks=Ks, ks=ks,
                objective=float(orc.final_obj))


@functools.lru_cache(maxsize=None)
def oracle_solves(name, perturbed=False, max_iter=MAX_ITER):
    """Every problem of the set through the oracle; perturbed: on (A, B) (1 + 1e-12 * standard normal), elementwise."""
    system, ab = matrices(name)
    d = problems(name)
    out = []
    for j, k in enumerate(d["index"]):
        A, B = ab[int(k)]
        if perturbed:
            rng = np.random.default_rng(7000 + j)
            A = A * (1.0 + 1e-12 * rng.normal(size=A.shape))
            B = B * (1.0 + 1e-12 * rng.normal(size=B.shape))
        out.append(oracle_solve(system, A, B, d["Q"][j], d["R"][j], d["F"][j], d["goal"][j], d["hz"][j], d["x0"][j],
                                max_iter))
    return out
