"""Training-data generators: the reference's ``autompc/utils/data_generation.py`` loops (uniform_random_generate
:13-29, random_walk_generate :55-75, periodic_control_generate :78-98, multisine_generate :100-137) with the same
signatures, plus ``device=``.

In all four the controls never depend on the state.  So ``state0`` and the controls are drawn from ``rng`` in the
reference's exact call order, trajectory by trajectory, the control arithmetic runs on the host exactly as the
reference writes it, and -- when ``dynamics`` is a ``DynamicsProgram`` and ``device`` is not False -- all trajectories
roll out in ONE ``ampc_program_rollout`` launch (one lane per trajectory).  Otherwise the reference's host loop runs:
``y = dynamics(y, u)`` step by step, interleaved with the draws as the reference interleaves them.  ``abort_if``
(multisine) truncates on the host afterwards on the device path.

``device``: False (default) host loop; True or "f64" the device in double precision; "f32" in single.
``prbs_generate`` is not mirrored: it hands the dynamics a scalar control.
"""
import numpy as np

from .sysid.program import DynamicsProgram
from .trajectory import Trajectory, zeros


def _state0(rng, init_min, init_max):
    return [rng.uniform(minval, maxval, 1)[0] for minval, maxval in zip(init_min, init_max)]


def _run(system, dynamics, traj_len, starts, device, abort_if=None):
    """starts: an iterator that draws, per trajectory, (state0, iterator over the traj_len controls) -- consumed in
    the reference's order: a trajectory's state0, then its controls one step at a time."""
    on_device = device is not False and device is not None
    if on_device and not isinstance(dynamics, DynamicsProgram):
        raise TypeError("device=%r needs the dynamics as a DynamicsProgram (DynamicsProgram.trace)" % (device,))
    trajs = []
    if not on_device:
        for state0, controls in starts:
            y = state0[:]
            traj = zeros(system, traj_len)
            traj.obs[:] = y
            for i in range(traj_len):
                traj[i].obs[:] = y
                u = next(controls)
                y = dynamics(y, u)
                traj[i].ctrl[:] = u
                if abort_if is not None and abort_if(y):
                    traj = traj[:i]
                    break
            trajs.append(traj)
        return trajs
    x0, ctrls = [], []
    for state0, controls in starts:
        x0.append(state0)
        U = np.empty((traj_len, system.ctrl_dim))
        for i in range(traj_len):
            U[i] = next(controls)
        ctrls.append(U)
    if not x0:
        return trajs
    x0 = np.array(x0, dtype=np.float64).reshape(len(x0), system.obs_dim)
    ctrls = np.array(ctrls, dtype=np.float64).reshape(len(x0), traj_len, system.ctrl_dim)
    obs = dynamics.rollout(x0, ctrls, device=True, precision="f32" if device == "f32" else "f64")
    for k in range(len(x0)):
        n = traj_len
        if abort_if is not None:
            for i in range(traj_len):
                if abort_if(obs[k, i + 1]):          # (the state AFTER step i, as the reference tests it)
                    n = i
                    break
        trajs.append(Trajectory(system, n, obs[k, :n].copy(), ctrls[k, :n].copy()))
    return trajs


def uniform_random_generate(system, task, dynamics, rng, init_min, init_max, traj_len, n_trajs, device=False):
    def starts():
        for _ in range(n_trajs):
            state0 = _state0(rng, init_min, init_max)
            umin, umax = task.get_ctrl_bounds().T

            def controls():
                while True:
                    yield rng.uniform(umin, umax, system.ctrl_dim)
            yield state0, controls()
    return _run(system, dynamics, traj_len, starts(), device)


def random_walk_generate(system, task, dynamics, rng, init_min, init_max, walk_rate, traj_len, n_trajs,
                         device=False):
    def starts():
        for _ in range(n_trajs):
            state0 = _state0(rng, init_min, init_max)
            umin, umax = task.get_ctrl_bounds().T
            uamp = np.min([umin, umax])
            u0 = rng.uniform(umin, umax, system.ctrl_dim)
            step_size = walk_rate * system.dt

            def controls(u=u0):
                while True:
                    u += uamp * step_size * rng.uniform(-1, 1, system.ctrl_dim)
                    u = np.clip(u, umin, umax)
                    yield u
            yield state0, controls()
    return _run(system, dynamics, traj_len, starts(), device)


def periodic_control_generate(system, task, dynamics, rng, init_min, init_max, U_1, traj_len, n_trajs,
                              device=False):
    periods = list(range(1, traj_len, max([1, traj_len // n_trajs])))

    def starts():
        for period in periods:
            state0 = _state0(rng, init_min, init_max)
            umin, umax = task.get_ctrl_bounds().T
            uamp = np.min([umin, umax])

            def controls(period=period):
                i = 0
                while True:
                    yield uamp * U_1 * np.cos(2 * np.pi * i / period)
                    i += 1
            yield state0, controls()
    return _run(system, dynamics, traj_len, starts(), device)


def multisine_generate(system, task, dynamics, rng, init_min, init_max, n_freqs, traj_len, n_trajs, abort_if=None,
                       device=False):
    periods = list(range(1, traj_len, n_freqs))
    umin, umax = task.get_ctrl_bounds().T
    uamp = (umax - umin) / 2
    umed = (umax + umin) / 2

    def starts():
        for _ in range(n_trajs):
            weights = []
            for i in range(system.ctrl_dim):
                vals = rng.uniform(size=len(periods) - 1)
                vals = np.concatenate([[0.0], np.sort(vals), [1.0]])
                weight = vals[1:] - vals[:-1]
                weights.append(weight)
            weights = np.array(weights)
            phases = rng.uniform(0, 2 * np.pi, len(periods))
            state0 = _state0(rng, init_min, init_max)

            def controls(weights=weights, phases=phases):
                i = 0
                while True:
                    u = np.zeros(system.ctrl_dim)
                    for j, period in enumerate(periods):
                        u += weights[:, j] * np.cos(2 * np.pi * i / period + phases[j])
                    yield uamp * u + umed
                    i += 1
            yield state0, controls()
    return _run(system, dynamics, traj_len, starts(), device, abort_if)
