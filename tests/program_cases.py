"""Shared cases of the DynamicsProgram tests (host, GPU) and of tests/golden/gen_golden_datagen.py: the dynamics
functions, written as benchmark dynamics are written, and the generator settings of the fixtures."""
import numpy as np

DT = 0.05


# -- CartPole-form dynamics, restated: sin, cos, division, in-place +=, u[0] and a passthrough component -----------
def cartpole_rates(y, u, g=9.8, m=1.0, L=0.7, b=0.4):
    theta, omega, x, dx = y
    return np.array([omega,
                     g * np.sin(theta) / L - b * omega / (m * L ** 2) + u * np.cos(theta) / L,
                     dx,
                     u])


def cartpole_step(y, u, dt=DT):
    y += dt * cartpole_rates(y, u[0])
    return y


def cartpole_system():
    from autompc_amd import System
    return System(["theta", "omega", "x", "dx"], ["u"], dt=DT)


# -- the fixtures' dynamics: two observations, two controls, returns a fresh array (takes lists too) ---------------
def pendulum2(y, u, dt=DT):
    th, om = y
    return np.array([th + dt * om,
                     om + dt * (-9.8 * np.sin(th) - 0.3 * om + u[0] + 0.5 * u[1] * np.cos(th))])


PEND_OBS, PEND_CTRL = ["th", "om"], ["u0", "u1"]
PEND_BOUNDS = {"u0": (-2.0, 1.5), "u1": (-1.0, 3.0)}
INIT_MIN, INIT_MAX = [-1.0, -0.5], [1.0, 0.5]
N_TRAJS, TRAJ_LEN = 3, 8
WALK_RATE, U_1, N_FREQS = 4.0, np.array([0.5, -0.25]), 2
ABORT_AT = 0.305                     # multisine_abort: stop once |th| exceeds this


def abort_if(y):
    return abs(y[0]) > ABORT_AT


def pendulum_system_task(System, Task):
    """With the project's classes, or with the reference's (the generator script)."""
    system = System(PEND_OBS, PEND_CTRL)
    system.dt = DT
    task = Task(system)
    for name, (lo, hi) in PEND_BOUNDS.items():
        task.set_ctrl_bound(name, lo, hi)
    return system, task


def generator_cases(mod, system, task, dynamics, **kw):
    """name -> list of trajectories, from the four generators of `mod` (ours, or the reference's)."""
    def rng(seed):
        return np.random.default_rng(seed)
    return {
        "uniform_random": mod.uniform_random_generate(system, task, dynamics, rng(11), INIT_MIN, INIT_MAX, TRAJ_LEN,
                                                      N_TRAJS, **kw),
        "random_walk": mod.random_walk_generate(system, task, dynamics, rng(12), INIT_MIN, INIT_MAX, WALK_RATE,
                                                TRAJ_LEN, N_TRAJS, **kw),
        "periodic": mod.periodic_control_generate(system, task, dynamics, rng(13), INIT_MIN, INIT_MAX, U_1, TRAJ_LEN,
                                                  N_TRAJS, **kw),
        "multisine": mod.multisine_generate(system, task, dynamics, rng(14), INIT_MIN, INIT_MAX, N_FREQS, TRAJ_LEN,
                                            N_TRAJS, **kw),
        "multisine_abort": mod.multisine_generate(system, task, dynamics, rng(15), INIT_MIN, INIT_MAX, N_FREQS,
                                                  TRAJ_LEN, N_TRAJS, abort_if=abort_if, **kw),
    }


# -- exact-arithmetic and transcendental programs for the device tests ---------------------------------------------
def exact_fn(y, u):
    """add / sub / mul / div / sqrt / abs / min / max / integer power only; a * b + c patterns invite contraction."""
    a, b, c = y
    p, q = u
    r0 = a * b + c                                   # would contract to one fma
    r1 = (a - p) * (b + q) - a * b
    r2 = np.sqrt(np.abs(c) + 1.5) / (np.abs(a) + 0.75)
    r3 = np.minimum(a, q) * np.maximum(b, p) + np.clip(c, -0.5, 0.5)
    return [r0 + r1 * r2, r3 ** 3 - r2 ** 2 + c ** -2 * 0.01, -(r1 ** 5) * 1e-3 + a / (b * b + 1.0)]


def smooth_fn(y, u):
    a, b, c = y
    p, q = u
    return [a + DT * (np.sin(b) * np.cos(c) + p),
            b + DT * (np.exp(-0.5 * a) - np.tanh(q * c)),
            np.tanh(a) * np.exp(0.25 * b) + np.cos(p) / (1.0 + c * c) + np.sin(q)]


def system_of(nx, nu):
    from autompc_amd import System
    return System(["x%d" % i for i in range(nx)], ["u%d" % i for i in range(nu)], dt=DT)


def exact_n(nx, nu):
    """Exact-arithmetic dynamics of any dimensions."""
    def fn(y, u):
        return [y[i] + DT * (y[(i + 1) % nx] * u[i % nu] - 0.5 * y[i]) / (abs(u[(i + 1) % nu]) + 1.0)
                for i in range(nx)]
    return fn


def smooth_n(nx, nu):
    def fn(y, u):
        return [y[i] + DT * (np.sin(y[(i + 1) % nx]) * u[i % nu] + np.cos(y[i]) - np.tanh(u[(i + 1) % nu]))
                + 0.01 * np.exp(-y[i] * y[i]) for i in range(nx)]
    return fn


def wide(n_live):
    """n_live values alive at once: n_live products, then their sum (n_live + 1 slots with the two inputs)."""
    def fn(y, u):
        terms = [y[0] * u[0] for _ in range(n_live)]
        acc = terms[0]
        for t in terms[1:]:
            acc = acc + t
        return [acc]
    return fn


def chain(n):
    """n instructions in two slots."""
    def fn(y, u):
        acc = y[0]
        for _ in range(n):
            acc = acc + u[0]
        return [acc]
    return fn


# -- closed loops: CartPole shape (4 observations, 1 control), an MLP as the controllers' model --------------------
def poly_step(y, u, dt=DT):
    """Exact arithmetic only: two coupled oscillators with a cubic spring."""
    a, da, b, db = y
    return [a + dt * da,
            da + dt * (u[0] - a - 0.5 * da - 0.2 * a ** 3 + 0.1 * b),
            b + dt * db,
            db + dt * (0.5 * u[0] - 0.3 * db - b)]


LOOP_INIT = np.array([0.3, 0.0, 0.1, -0.1])
LOOP_STEPS = 10
LOOP_UMAX = 1.5


def loop_task(system, term_cond=None):
    from autompc_amd import QuadCost, Task
    task = Task(system)
    task.set_cost(QuadCost(system, np.eye(4), 0.1 * np.eye(1), 2.0 * np.eye(4)))
    task.set_ctrl_bounds([-LOOP_UMAX], [LOOP_UMAX])
    task.set_init_obs(LOOP_INIT)
    task.set_num_steps(LOOP_STEPS)
    if term_cond is not None:
        task.set_term_cond(term_cond)
    return task


def loop_mlp_params(seed=5, hidden=(32, 32)):
    from oracle import mlp as omlp
    return omlp.random_params(4, 1, list(hidden), "tanh", seed=seed)


def mppi_cands():
    return [dict(horizon=5 + b, sigma=0.2 + 0.1 * b, lmda=1.0 + 0.25 * b, num_path=16 + 8 * b,
                 Q=np.full(4, 1.0 + 0.5 * b), R=np.full(1, 0.2), F=np.full(4, 2.0)) for b in range(3)]


def mppi_noise(cands, T, seed=9):
    rng = np.random.default_rng(seed)
    acts = [rng.normal(scale=np.sqrt(c["sigma"]), size=(c["horizon"], 1)) for c in cands]
    eps = [[rng.normal(scale=np.sqrt(c["sigma"]), size=(c["num_path"], c["horizon"], 1)) for c in cands]
           for _ in range(T)]
    return acts, eps


def oracle_mppi_loops(system, p_ctl, cands, acts, eps, T, step):
    """Every candidate's closed loop with the oracle MPPI stepped on the host and `step(x, u)` as the dynamics:
    list of (obs [T+1][4], ctrls [T+1][1])."""
    from oracle.costs import QuadCostOracle
    from oracle.mlp import MLPOracle
    from oracle.mppi import MPPIOracle
    out = []
    for b, c in enumerate(cands):
        np.random.seed(0)
        orc = MPPIOracle(MLPOracle(system, p_ctl),
                         QuadCostOracle(np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), np.zeros(4)),
                         np.array([[-LOOP_UMAX, LOOP_UMAX]]), horizon=c["horizon"], num_path=c["num_path"],
                         sigma=c["sigma"], lmda=c["lmda"])
        orc.act_sequence = acts[b].copy()
        x, cs = LOOP_INIT.copy(), np.concatenate([LOOP_INIT, np.zeros(1)])
        o_obs, o_ctl = [x.copy()], []
        for s in range(T):
            u, cs = orc.run(cs, x, eps_nhu=eps[s][b])
            x = np.asarray(step(x, u), dtype=np.float64)
            o_ctl.append(u)
            o_obs.append(x.copy())
        o_ctl.append(np.zeros(1))
        out.append((np.array(o_obs), np.array(o_ctl)))
    return out
