"""Shared cases of the tests of iLQR on analytic dynamics programs (host, GPU): the solve cases A..D, their oracle
(oracle.ilqr.ILQROracle on the DifferentiableProgram's host methods) with the margins of its decisions, the per-
iteration step index of a device solve, and the plan's LDS map restated.

Inputs.  Every case's oracle keeps, in every iteration, at least MARGIN = 1e-6 between each quantity it decides on and
its threshold (``margins`` below; tests/test_program_ilqr_host.py asserts it on this CPU, the oracle alone): the
device's 1e-12-level deviations cannot flip a decision.  Case C's x0 is rng(SEED_C) uniform in +-0.5 and case D's
rng(SEED_D) uniform in +-0.5 -- the seeds at which the oracle takes 11 / 11 / 15 / 14 iterations with step indices up
to 7 and active clipping (C) and 21 iterations for the full solve (D); case A uses the inputs of the SINDy iLQR test,
case B the closed loops' task (program_cases.loop_task: its cost, its bounds, LOOP_INIT).  None had to be moved."""
import numpy as np

import program_cases as C
from autompc_amd.sysid.program import DifferentiableProgram

MARGIN = 1e-6
SEED_C, SEED_D = 67, 40
X0_A = np.array([0.3, -0.2, 0.1, 0.0])


def quad(nx, nu):
    """Q, R, F of every solve case (those of the SINDy iLQR test)."""
    return np.eye(nx), 0.1 * np.eye(nu), 5.0 * np.eye(nx)


def program(name, ilqr=True):
    if name == "cartpole":
        return DifferentiableProgram.trace(C.cartpole_system(), C.cartpole_step, ilqr=ilqr)
    if name == "poly_step":
        return DifferentiableProgram.trace(C.cartpole_system(), C.poly_step, ilqr=ilqr)
    if name == "exact_n(17,6)":
        return DifferentiableProgram.trace(C.system_of(17, 6), C.exact_n(17, 6), ilqr=ilqr)
    if name == "smooth_n(62,1)":
        return DifferentiableProgram.trace(C.system_of(62, 1), C.smooth_n(62, 1), ilqr=ilqr)
    if name == "smooth_n(53,1)":
        return DifferentiableProgram.trace(C.system_of(53, 1), C.smooth_n(53, 1), ilqr=ilqr)
    raise KeyError(name)


EXACT = ("poly_step", "exact_n(17,6)")        # programs whose instructions all round exactly: bit-for-bit on the device


def solve_cases():
    """id -> dict(prog, H, x0, guess, bounds (lo, hi) or None, max_iter)."""
    cases = {}
    for H in (1, 2, 15):
        for bounds in (None, (-0.4, 0.6)):
            cases["A-H%d-%s" % (H, "bounded" if bounds else "free")] = dict(
                prog="cartpole", H=H, x0=X0_A, guess=np.zeros((H, 1)), bounds=bounds, max_iter=50)
    cases["B-H15"] = dict(prog="poly_step", H=15, x0=C.LOOP_INIT.copy(), guess=np.zeros((15, 1)),
                          bounds=(-C.LOOP_UMAX, C.LOOP_UMAX), max_iter=50, F=2.0 * np.eye(4))
    x0c = np.random.default_rng(SEED_C).uniform(-0.5, 0.5, 17)
    for H in (3, 9):
        for bounds in (None, (-0.5, 0.5)):
            cases["C-H%d-%s" % (H, "bounded" if bounds else "free")] = dict(
                prog="exact_n(17,6)", H=H, x0=x0c, guess=np.full((H, 6), 0.3), bounds=bounds, max_iter=50)
    cases["D-H4"] = dict(prog="smooth_n(62,1)", H=4, x0=np.random.default_rng(SEED_D).uniform(-0.5, 0.5, 62),
                         guess=np.zeros((4, 1)), bounds=None, max_iter=3)
    # D's 62 states are past the full LDS map (plan_lds_bytes below): it runs on the compact one.  E is D at 53 states,
    # the largest smooth_n(n, 1) whose plan fits the full map -- the sweep and the helper loops for nx > 32
    cases["E-H4"] = dict(prog="smooth_n(53,1)", H=4, x0=np.random.default_rng(SEED_D).uniform(-0.5, 0.5, 53),
                         guess=np.zeros((4, 1)), bounds=None, max_iter=3)
    return cases


def ubounds(case, nu):
    if case["bounds"] is None:
        return None
    return np.full(nu, case["bounds"][0]), np.full(nu, case["bounds"][1])


def case_oracle(prog, case):
    return make_oracle(prog, case["H"], ubounds(case, prog.system.ctrl_dim), case["max_iter"], F=case.get("F"))


def case_task(prog, case):
    """The Task of a case for the drop-in controller."""
    from autompc_amd import QuadCost, Task
    nx, nu = prog.system.obs_dim, prog.system.ctrl_dim
    q, r, f = quad(nx, nu)
    task = Task(prog.system)
    task.set_cost(QuadCost(prog.system, q, r, f if case.get("F") is None else case["F"]))
    if case["bounds"] is not None:
        task.set_ctrl_bounds([case["bounds"][0]] * nu, [case["bounds"][1]] * nu)
    return task


def make_oracle(prog, H, ub=None, max_iter=50, Q=None, R=None, F=None):
    """A MarginOracle (below) on the program's host methods with the quadratic cost of `quad` (or Q, R, F)."""
    from oracle.costs import QuadCostOracle
    nx, nu = prog.system.obs_dim, prog.system.ctrl_dim
    q, r, f = quad(nx, nu)
    cost = QuadCostOracle(q if Q is None else Q, r if R is None else R, f if F is None else F, np.zeros(nx))
    return _margin_oracle_class()(prog, cost, prog.system.dt, H, ubounds=ub, max_iter=max_iter)


def _margin_oracle_class():
    from oracle.ilqr import ILQROracle

    class MarginOracle(ILQROracle):
        """ILQROracle that keeps what every iteration decided on: the sweep's (lin, quad, |ks|) and the line search's
        candidates with the nominal controls they started from."""

        def solve(self, x0, uguess):
            self.sweeps, self.searches = [], []
            return super().solve(x0, uguess)

        def _backward(self, states, ctrls, Jacs):
            out = super()._backward(states, ctrls, Jacs)
            self.sweeps.append((out[2], out[3], float(np.linalg.norm(out[1]))))
            return out

        def _line_search_rollout(self, x0, states, ctrls, Ks, ks, alphas):
            out = super()._line_search_rollout(x0, states, ctrls, Ks, ks, alphas)
            self.searches.append((out[0].copy(), out[1].copy(), np.array(ctrls, copy=True), np.array(alphas)))
            return out

        def step_indices(self):
            """The candidate each iteration swapped in (trace: best index on success, else the last one evaluated);
            the final iteration of a solve that stopped on the failure test swapped nothing: -1."""
            out = []
            for k, (obj, new_obj, best, success, last) in enumerate(self.trace):
                stopped = (not success and new_obj > obj + 1e-3) or best < 0
                out.append(-1 if stopped else (best if success else last))
            return out

        def clipped(self):
            """Did any accepted candidate sit on a bound?"""
            if self.ubounds is None:
                return False
            hit = False
            for (ls_states, ls_ctrls, _, _), j in zip(self.searches, self.step_indices()):
                if j >= 0:
                    hit = hit or bool(np.any(ls_ctrls[j] <= self.ubounds[0]) or np.any(ls_ctrls[j] >= self.ubounds[1]))
            return hit

        def margins(self):
            """The smallest distance, over every decision of the last solve that its outcome depends on, between what
            was compared: the ratio against ls_cost_threshold; best_obj against obj (relative to |obj|) where no
            candidate passed the ratio test -- one that passes has obj - new_obj = ratio * (-expect) > 0 with the
            ratio's margin; |ks| and |du| against u_threshold (relative to it).  An iteration whose |ks| is below
            u_threshold evaluates candidate 0 only and swaps it in whatever the ratio and the objectives say (both
            are differences of equal numbers then): only its |ks| and |du| count.  So do those of an iteration all of
            whose candidates ARE the nominal trajectory, control for control, bit for bit (every control on the bound
            it was on: cases A-H2 and A-H15 bounded end this way): each side compares a number with itself, whatever
            it picks is the same trajectory, and |du| = 0 ends the solve."""
            worst = {"ratio": np.inf, "best_obj": np.inf, "ks_norm": np.inf, "du_norm": np.inf}
            for (lin, quad_, ksn), (ls_states, ls_ctrls, ctrls, alphas), tr, sel in zip(self.sweeps, self.searches,
                                                                                        self.trace, self.step_indices()):
                obj, _, best, success, last = tr
                best_obj, passed = np.inf, False
                same = all(np.array_equal(ls_ctrls[j], ctrls) for j in range(last + 1))
                decides = ksn >= self.u_threshold and not same
                for j in range(last + 1 if decides else 0):
                    new_obj = self._objective(ls_states[j], ls_ctrls[j])
                    ratio = (obj - new_obj) / -(alphas[j] * lin + alphas[j] ** 2 * quad_ / 2)
                    worst["ratio"] = min(worst["ratio"], abs(ratio - self.ls_cost_threshold))
                    if ratio > self.ls_cost_threshold:
                        passed = True
                        break
                    best_obj = min(best_obj, new_obj)
                if decides and not passed:
                    worst["best_obj"] = min(worst["best_obj"], abs(best_obj - obj) / max(abs(obj), 1e-300))
                worst["ks_norm"] = min(worst["ks_norm"], abs(ksn - self.u_threshold) / self.u_threshold)
                if sel >= 0:
                    du = float(np.linalg.norm(ls_ctrls[sel] - ctrls))
                    worst["du_norm"] = min(worst["du_norm"], abs(du - self.u_threshold) / self.u_threshold)
            return worst

    return MarginOracle


def device_step_indices(plan, orc, x0, guess, n_iter, tol=1e-9):
    """The candidates the device may have swapped in at every iteration, recovered from its own results: the solve is
    run with max_iter = 0 .. n_iter (deterministic: the first k iterations of every run are the same), and iteration
    k's candidates are rebuilt on the host from the device's gains of that iteration and its nominal trajectory before
    it.  Per iteration: the indices of the candidates whose controls are the device's new controls -- the closest one,
    within tol, and those bit-identical to it on the host (controls all on their bounds); every other candidate must
    be at least a thousand times further away.  An iteration whose |ks| is below u_threshold evaluates candidate 0
    only (its candidates lie within |ks| of each other): it must be candidate 0, within tol."""
    from oracle.ilqr import ILQROracle
    alphas = np.array([orc.ls_discount ** i for i in range(orc.ls_max_iter)])
    prev = plan.solve(x0[None], guess[None], 0)
    out = []
    for k in range(1, n_iter + 1):
        cur = plan.solve(x0[None], guess[None], k)
        _, ls_ctrls = ILQROracle._line_search_rollout(orc, x0, prev["states"][0], prev["ctrls"][0], cur["Ks"][0],
                                                      cur["ks"][0], alphas)
        d = np.abs(ls_ctrls - cur["ctrls"][0][None]).reshape(len(alphas), -1).max(axis=1)
        if np.linalg.norm(cur["ks"][0]) < orc.u_threshold:
            assert d[0] <= tol, (k, d)
            out.append([0])
            prev = cur
            continue
        j = int(np.argmin(d))
        assert d[j] <= tol, (k, d)
        match = [i for i in range(len(alphas)) if np.array_equal(ls_ctrls[i], ls_ctrls[j])]
        assert all(d[i] >= 1000 * max(d[j], 1e-15) for i in range(len(alphas)) if i not in match), (k, d)
        out.append(match)
        prev = cur
    return out


# -- the plan's LDS map (csrc/api_ilqr.cpp: ilqr_plan_build, csrc/ilqr_kernels.hpp: make_ilqr_work), in f64 values -----
LDS_LIMIT = 160 * 1024


def cost_block_stride(no, nu):
    """csrc/mlp_tile.hpp: Q, R, F, goal, lin, lint and the two constants, padded to four values."""
    n = 2 * no * no + nu * nu + 3 * no + 2
    return (n + 3) // 4 * 4


def ilqr_work_total(nx, nu, cost_stride):
    n = nx + nu
    return (nx * nx + nx + 2 * nx * n + n * n + n + nu * nx + nu + nu * nx + nu + nu * nu + nu * (nx + 1) + nx + nu
            + cost_stride + 2 * nu + 16 + 16 + (nu + 1) // 2 + 8)


def ilqr_compact_total(nx, nu, cost_stride):
    """make_ilqr_work(.., compact = true): what the line search itself touches."""
    return nu * nx + nu + nu + nu * nu + nx + nu + cost_stride + 2 * nu + 16 + 16 + (nu + 1) // 2 + 8


def plan_compact_bytes(nx, nu, n_slots, cost_stride):
    """(line search, sweep) bytes of the second tier, taken by plans whose plan_lds_bytes is past the limit: the rows,
    next states and slots with the compact workspace; the sweep's workspace without the cost block."""
    up4 = lambda v: (v + 3) // 4 * 4
    work = up4(up4(16 * (nx + nu + 1)) + 16 * nx + 16 * n_slots)
    return 8 * (work + ilqr_compact_total(nx, nu, cost_stride)), 8 * ilqr_work_total(nx, nu, 0)


def plan_lds_bytes(nx, nu, n_slots, cost_stride):
    """[16][nx + nu + 1] rows | [16][nx] next states | [n_slots][16] slots (each region padded to four values), then
    the Riccati / line-search workspace."""
    up4 = lambda v: (v + 3) // 4 * 4
    lds_xn = up4(16 * (nx + nu + 1))
    work = up4(lds_xn + 16 * nx + 16 * n_slots)
    return 8 * (work + ilqr_work_total(nx, nu, cost_stride))
