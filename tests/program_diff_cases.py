"""Shared cases of the DifferentiableProgram tests (host, GPU): the traced programs, raw programs around the kinks of
abs / min / max and the integer powers, and inputs away from the kinks."""
import numpy as np

import program_cases as C
from autompc_amd.sysid import program as P

POWERS = (0, 1, 2, 3, -1, -2, 64, -64)


def traced(cls):
    """name -> program of class `cls`, for the six functions of program_cases.py."""
    return {
        "cartpole": cls.trace(C.cartpole_system(), C.cartpole_step),
        "exact_fn": cls.trace(C.system_of(3, 2), C.exact_fn),
        "smooth_fn": cls.trace(C.system_of(3, 2), C.smooth_fn),
        "poly_step": cls.trace(C.cartpole_system(), C.poly_step),
        "exact_n(17,6)": cls.trace(C.system_of(17, 6), C.exact_n(17, 6)),
        "smooth_n(17,6)": cls.trace(C.system_of(17, 6), C.smooth_n(17, 6)),
    }


def away_from_kinks(nx, nu, n, seed=0):
    """Inputs of magnitude 0.3 .. 1.5 with random signs."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.3, 1.5, (n, nx)) * rng.choice([-1.0, 1.0], (n, nx))
    U = rng.uniform(0.3, 1.5, (n, nu)) * rng.choice([-1.0, 1.0], (n, nu))
    return X, U


def abs_program(cls):
    """x' = |x| * u  (nx = nu = 1)."""
    return cls.from_code(C.system_of(1, 1), [[P.OP_ABS, 2, 0, 0], [P.OP_MUL, 2, 2, 1]], [], [2])


def minmax_program(cls):
    """x0' = min(x0, x1) * u, x1' = max(x0, x1) * u  (nx = 2, nu = 1)."""
    return cls.from_code(C.system_of(2, 1), [[P.OP_MIN, 3, 0, 1], [P.OP_MAX, 4, 0, 1], [P.OP_MUL, 3, 3, 2],
                                             [P.OP_MUL, 4, 4, 2]], [], [3, 4])


def powi_program(cls, n):
    """x' = x ** n + u  (nx = nu = 1)."""
    return cls.from_code(C.system_of(1, 1), [[P.OP_POWI, 2, 0, n], [P.OP_ADD, 2, 2, 1]], [], [2])


def kink_rows():
    """(program builder, states, ctrls) with rows on, below and above every kink."""
    return [
        (abs_program, np.array([[-0.75], [0.0], [1.25]]), np.array([[2.0], [2.0], [-0.5]])),
        (minmax_program, np.array([[0.25, 0.5], [0.5, 0.25], [0.375, 0.375]]), np.array([[1.5], [-2.0], [3.0]])),
    ]


def jvp_at_slot_limit():
    """(nx, nu, n_slots, code, consts, out_slot) of a raw JVP program for nx = nu = 1 that uses all 256 slots: slot 4
    is x + u, every slot after it the slot before plus x; the value output is the last of them, the tangent output
    dx + du."""
    code = [[P.OP_ADD, 4, 0, 1]]
    for s in range(5, P.MAX_SLOTS):
        code.append([P.OP_ADD, s, s - 1, 0])
    code.append([P.OP_ADD, 2, 2, 3])
    return 1, 1, P.MAX_SLOTS, np.array(code, dtype=np.int32), np.zeros(0), np.array([P.MAX_SLOTS - 1, 2], dtype=np.int32)


def wide_state_program():
    """(code, consts, out_slot, jvp_code, jvp_out_slot) of x0' = x0 + u, x_i' = x_i for nx = 64, nu = 1, written so
    that the program and its JVP (130 inputs) both name slot 255: n_slots = 256 each."""
    code = np.array([[P.OP_ADD, 255, 0, 64]], dtype=np.int32)
    out = np.array([255] + list(range(1, 64)), dtype=np.int32)
    jcode = np.array([[P.OP_ADD, 255, 0, 64], [P.OP_ADD, 254, 65, 129]], dtype=np.int32)
    jout = np.array([255] + list(range(1, 64)) + [254] + list(range(66, 129)), dtype=np.int32)
    return code, np.zeros(0), out, jcode, jout


def oracle_program_loops(prog, cands, acts, eps, T, umax=C.LOOP_UMAX, init=C.LOOP_INIT):
    """Every candidate's closed loop with the oracle MPPI planning on `prog` (its host pred_batch) and `prog` stepped
    on the host as the dynamics: list of (obs [T+1][4], ctrls [T+1][1]) -- program_cases.oracle_mppi_loops with the
    program in the MLP's place."""
    from oracle.costs import QuadCostOracle
    from oracle.mppi import MPPIOracle
    out = []
    for b, c in enumerate(cands):
        np.random.seed(0)
        orc = MPPIOracle(prog, QuadCostOracle(np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), np.zeros(4)),
                         np.array([[-umax, umax]]), horizon=c["horizon"], num_path=c["num_path"], sigma=c["sigma"],
                         lmda=c["lmda"])
        orc.act_sequence = acts[b].copy()
        x, cs = init.copy(), np.concatenate([init, np.zeros(1)])
        o_obs, o_ctl = [x.copy()], []
        for s in range(T):
            u, cs = orc.run(cs, x, eps_nhu=eps[s][b])
            x = np.asarray(prog.pred(x, u), dtype=np.float64)
            o_ctl.append(u)
            o_obs.append(x.copy())
        o_ctl.append(np.zeros(1))
        out.append((np.array(o_obs), np.array(o_ctl)))
    return out
