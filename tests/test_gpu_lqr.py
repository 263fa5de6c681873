"""Finite-horizon LQR on the device (ampc_lqr_*, control/lqr.py) against the reference's goldens
(tests/golden/gen_golden_lqr.py)."""
import os

import numpy as np
import pytest

from autompc_amd import ARX, MLP, Koopman, QuadCost, SumCost, System, Task, simulate, zeros
from autompc_amd import _lib
from autompc_amd.control.lqr import LQR, FiniteHorizonLQR
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def gold(name):
    return np.load(os.path.join(GOLD, "lqr_%s.npz" % name))


def riccati(A, B, Q, R, F, horizon):
    """The reference's recursion (lqr.py:15-47, N = 0) in numpy, Q and F padded."""
    n = A.shape[0]
    Qp, Fp = np.zeros((n, n)), np.zeros((n, n))
    Qp[:Q.shape[0], :Q.shape[1]] = Q
    Fp[:F.shape[0], :F.shape[1]] = F
    P = Fp
    for _ in range(horizon + 1):
        P = A.T @ P @ A - (A.T @ P @ B) @ np.linalg.inv(R + B.T @ P @ B) @ (B.T @ P @ A) + Qp
    return -np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A)


def system(no, nu):
    return System(["x%d" % i for i in range(no)], ["u%d" % i for i in range(nu)], dt=0.05)


def arx_of(g, no, nu):
    m = ARX(system(no, nu), history=int(g["history"]))
    m.set_parameters({"coeffs": g["coeffs"]})
    return m


def task_of(g, sys_):
    t = Task(sys_)
    t.set_cost(QuadCost(sys_, g["Q"], g["R"], g["F"], goal=g["goal"]))
    if np.all(np.isfinite(g["umax"])):
        t.set_ctrl_bounds(g["umin"], g["umax"])
    return t


def seeded_mlp(sys_, hidden, activation, seed):
    no, nu = sys_.obs_dim, sys_.ctrl_dim
    p = omlp.random_params(no, nu, hidden, activation, seed=seed)
    rng = np.random.default_rng(seed + 7919)               # gen_golden.normalisers
    p["xu_means"], p["xu_std"] = rng.normal(scale=0.3, size=no + nu), rng.uniform(0.5, 2.0, size=no + nu)
    p["dy_means"], p["dy_std"] = rng.normal(scale=0.02, size=no), rng.uniform(0.05, 0.2, size=no)
    m = MLP(sys_, n_hidden_layers=len(hidden), hidden_size=hidden[0], nonlintype=activation)
    m.weights, m.biases = p["weights"], p["biases"]
    m.xu_means, m.xu_std, m.dy_means, m.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
    return m


# The numpy recursion restated here (it solves where the reference inverts) agrees with the reference's goldens
# to at most 7.3e-16 of max|K| over every case below, horizons 1..1000: the recursion does not amplify rounding.
# GAIN_NUMPY_TOL bounds that; the device sums in its own fixed order and gets a hundred times more room.
GAIN_NUMPY_TOL = 1e-14
GAIN_TOL = 1e-12
CASES = [("arx2_small", 4, 1), ("sumcost", 4, 1), ("arx4_mlp", 17, 6), ("arx10_wide", 17, 6)]


@pytest.mark.parametrize("name,no,nu", CASES)
def test_gain_parity(name, no, nu):
    g = gold(name)
    m = arx_of(g, no, nu)
    A, B = m.to_linear()
    hs = [int(h) for h in g["horizons"]]
    plan = _lib.LqrPlan([_handle(m)] * len(hs), no, nu)
    K, status = plan.gains(hs, g["Q"], g["R"], g["F"])
    assert np.all(status == 0)
    for i, h in enumerate(hs):
        ref = g["K_%d" % h]
        scale = np.abs(ref).max()
        assert np.abs(riccati(A, B, g["Q"], g["R"], g["F"], h) - ref).max() / scale < GAIN_NUMPY_TOL
        assert np.abs(K[i] - ref).max() / scale < GAIN_TOL, (name, h)
    plan.close()


def _handle(model):
    h = _lib.Handle(0, "f64")
    A, B = model.to_linear()
    h.set_linear(A, B)
    return h


def test_sumcost_matrices_are_summed():
    g = gold("sumcost")
    np.testing.assert_array_equal(g["Q"], g["Q1"] + g["Q2"])
    s = system(4, 1)
    cost = SumCost(s, [QuadCost(s, g["Q1"], g["R1"], g["F1"], goal=g["goal"]),
                       QuadCost(s, g["Q2"], g["R2"], g["F2"], goal=g["goal"])])
    t = Task(s)
    t.set_cost(cost)
    ctl = LQR(s, t, arx_of(g, 4, 1), "true", 10)
    assert np.abs(ctl.K - g["K_10"]).max() / np.abs(g["K_10"]).max() < GAIN_TOL


def test_singular_gain():
    g = gold("singular")
    assert int(g["raised"]) == 1
    s = system(3, 2)
    m = ARX(s, history=int(g["history"]))
    m.set_parameters({"coeffs": g["coeffs"]})
    plan = _lib.LqrPlan([_handle(m)], 3, 2)
    K, status = plan.gains([int(g["horizon"])], g["Q"], g["R"], g["F"])
    assert status[0] == 1 and np.all(np.isnan(K[0]))
    t = Task(s)
    t.set_cost(QuadCost(s, g["Q"], g["R"], g["F"]))
    with pytest.raises(np.linalg.LinAlgError):
        FiniteHorizonLQR(s, t, m, int(g["horizon"]))


def _dropin_case(name):
    g = gold(name)
    if name == "koop_mlp":
        s = system(4, 1)
        m = Koopman(s, method="lstsq", poly_basis=True, poly_degree=int(g["poly_degree"]))
        m.set_parameters({"A": g["A"], "B": g["B"]})
        sur = seeded_mlp(s, [int(v) for v in g["sur_hidden"]], "relu", int(g["sur_seed"]))
    else:
        no, nu = (4, 1) if name == "arx2_small" else (17, 6)
        s = system(no, nu)
        m = arx_of(g, no, nu)
        sur = seeded_mlp(s, [int(v) for v in g["sur_hidden"]], "tanh", int(g["sur_seed"])) if "sur_seed" in g else m
    return g, s, m, sur


# closed loops compound rounding over the episode: trajectories within 1e-8 of max|obs|
TRAJ_TOL = 1e-8


@pytest.mark.parametrize("name", ["arx2_small", "arx4_mlp", "koop_mlp", "arx10_wide"])
def test_dropin_closed_loop(name):
    g, s, m, sur = _dropin_case(name)
    t = task_of(g, s)
    for h in [int(v) for v in g["horizons"]]:
        ctl = LQR(s, t, m, "true", h)
        t0 = zeros(s, 1)
        t0[0].obs[:] = g["init_obs"]
        np.testing.assert_allclose(ctl.traj_to_state(t0), g["cstate0_%d" % h], rtol=0, atol=1e-14)
        n = g["obs_%d" % h].shape[0] - 1
        traj = simulate(ctl, g["init_obs"], sim_model=sur, max_steps=n, silent=True)
        ref_o, ref_c = g["obs_%d" % h], g["ctrls_%d" % h]
        assert np.abs(traj.obs - ref_o).max() / np.abs(ref_o).max() < TRAJ_TOL, (name, h)
        assert np.abs(traj.ctrls - ref_c).max() / max(np.abs(ref_c).max(), 1e-12) < TRAJ_TOL, (name, h)


def _device_loop(name, h):
    g, s, m, sur = _dropin_case(name)
    no, nu = s.obs_dim, s.ctrl_dim
    hm = _handle(m)
    hs = _lib.Handle(0, "f64")
    sur.stage_into(hs)
    plan = _lib.LqrPlan([hm], no, nu)
    K, st = plan.gains([h], g["Q"], g["R"], g["F"])
    rule = 2 if name == "koop_mlp" else 1
    lift = [m.device_lift()] if rule == 2 else None
    plan.set_loop([rule], g["goal"], g["umin"], g["umax"], lifts=lift)
    t0 = zeros(s, 1)
    t0[0].obs[:] = g["init_obs"]
    n = g["obs_%d" % h].shape[0] - 1
    obs, ctl = plan.closed_loop(hs, [m.traj_to_state(t0)], sur.traj_to_state(t0)[None], n)
    return g, obs[0], ctl[0]


@pytest.mark.parametrize("name", ["arx2_small", "arx4_mlp", "koop_mlp", "arx10_wide"])
def test_device_closed_loop_matches_reference(name):
    g = gold(name)
    for h in [int(v) for v in g["horizons"]]:
        _, o, c = _device_loop(name, h)
        ref_o, ref_c = g["obs_%d" % h], g["ctrls_%d" % h]
        assert np.abs(o - ref_o).max() / np.abs(ref_o).max() < TRAJ_TOL, (name, h)
        assert np.abs(c - ref_c).max() / max(np.abs(ref_c).max(), 1e-12) < TRAJ_TOL, (name, h)


def test_limits_refused():
    s = system(4, 1)
    mlp = seeded_mlp(s, [16], "relu", 5)
    hm = _lib.Handle(0, "f64")
    h32 = _lib.Handle(0, "f32")
    hl = _handle(_trained_arx(s, 2, 1))
    try:
        mlp.stage_into(hm)
        with pytest.raises(_lib.AmpcError, match="linear model"):
            _lib.LqrPlan([hm], 4, 1)
        h32.set_linear(np.eye(4), np.ones((4, 1)))
        with pytest.raises(_lib.AmpcError, match="f64"):
            _lib.LqrPlan([h32], 4, 1)
        with pytest.raises(_lib.AmpcError, match="ctrl_dim"):
            _lib.LqrPlan([hl], 4, 17)
        with pytest.raises(_lib.AmpcError, match="obs_dim"):
            _lib.LqrPlan([hl], 257, 1)
        plan = _lib.LqrPlan([hl], 4, 1)
        with pytest.raises(_lib.AmpcError, match="1..1000"):
            plan.gains([1001], np.eye(4), np.eye(1), np.eye(4))
        plan.close()
        t = Task(s)
        t.set_cost(QuadCost(s, np.eye(4), np.eye(1), np.eye(4)))
        with pytest.raises(TypeError, match="linear model"):
            LQR(s, t, mlp, "true", 10)
    finally:
        for h in (hm, h32, hl):
            h.close()


def test_restaged_model_refused():
    s = system(4, 1)
    h = _handle(_trained_arx(s, 2, 1))
    plan = _lib.LqrPlan([h], 4, 1)
    plan.gains([10], np.eye(4), np.eye(1), np.eye(4))
    big = _trained_arx(s, 3, 1)
    h.set_linear(*big.to_linear())                  # another state dimension
    with pytest.raises(_lib.AmpcError, match="re-staged"):
        plan.gains([10], np.eye(4), np.eye(1), np.eye(4))
    with pytest.raises(_lib.AmpcError, match="re-staged"):
        plan.set_loop([1], np.zeros(4), -np.ones(1), np.ones(1))
    plan.close()
    h.close()


# ---- batches: mixed state dimensions and horizons in one plan -------------------------------------------
def _training_trajs(s, seed, n=6, L=60):
    """Seeded stable linear system with noise (as gen_golden_lqr.training_trajs)."""
    from autompc_amd import Trajectory
    rng = np.random.default_rng(seed)
    no, nu = s.obs_dim, s.ctrl_dim
    A = 0.9 * np.linalg.qr(rng.normal(size=(no, no)))[0]
    B = 0.3 * rng.normal(size=(no, nu))
    out = []
    for _ in range(n):
        obs, ctl = np.zeros((L, no)), rng.normal(size=(L, nu))
        x = rng.normal(size=no)
        for i in range(L):
            obs[i] = x
            x = A @ x + B @ ctl[i] + 0.01 * rng.normal(size=no)
        out.append(Trajectory(s, L, obs, ctl))
    return out


def _trained_arx(s, history, seed):
    m = ARX(s, history=history)
    m.train(_training_trajs(s, seed))
    return m


def _mixed_batch(B, seed):
    """B problems on a 6-observation / 2-control system: ARX histories 1..10 (7..79 states, both sides of the
    kernel's 64-wide tile), horizons 1..1000 (1 and 1000 included), random diagonal costs."""
    s = system(6, 2)
    models = [_trained_arx(s, k, 20 + k) for k in range(1, 11)]
    rng = np.random.default_rng(seed)
    hist = rng.integers(0, 10, B)
    hist[:10] = np.arange(10)
    hz = rng.integers(1, 1001, B)
    hz[:3] = [1, 1000, 1000]
    Q = np.array([np.diag(10 ** rng.uniform(-1, 1, 6)) for _ in range(B)])
    R = np.array([np.diag(10 ** rng.uniform(-1, 1, 2)) for _ in range(B)])
    F = np.array([np.diag(10 ** rng.uniform(-1, 1, 6)) for _ in range(B)])
    return s, models, hist, hz, Q, R, F


# The batch's random costs condition R + B'PB less well than the goldens: two valid association orders of the same
# recursion in numpy (the reference's, and the device's P [A | B] then [A | B]'M) differ by up to 2.6e-11 of max|K|
# on this batch (measured).  The device against the reference's order: MIXED_GAIN_TOL.
MIXED_GAIN_TOL = 1e-9


def test_mixed_batch_gains_independent_of_the_batch():
    B = 64
    s, models, hist, hz, Q, R, F = _mixed_batch(B, 3)
    handles = [_handle(m) for m in models]
    plan = _lib.LqrPlan([handles[k] for k in hist], 6, 2)
    K, st = plan.gains(hz, Q, R, F)
    assert np.all(st == 0)
    assert len({k.shape[1] for k in K}) == 10 and max(k.shape[1] for k in K) > 64
    for i in range(B):                         # the reference's recursion, problem by problem
        A, Bm = models[hist[i]].to_linear()
        ref = riccati(A, Bm, Q[i], R[i], F[i], int(hz[i]))
        assert np.abs(K[i] - ref).max() / np.abs(ref).max() < MIXED_GAIN_TOL, i
    for i in range(B):                         # alone: the same bits
        one = _lib.LqrPlan([handles[hist[i]]], 6, 2)
        Ki, _ = one.gains(hz[i:i + 1], Q[i:i + 1], R[i:i + 1], F[i:i + 1])
        assert np.array_equal(Ki[0], K[i]), i
        one.close()
    perm = np.random.default_rng(4).permutation(B)
    pp = _lib.LqrPlan([handles[hist[i]] for i in perm], 6, 2)
    Kp, _ = pp.gains(hz[perm], Q[perm], R[perm], F[perm])
    for j, i in enumerate(perm):
        assert np.array_equal(Kp[j], K[i])
    for lo, hi in ((0, 23), (23, B)):
        sp = _lib.LqrPlan([handles[hist[i]] for i in range(lo, hi)], 6, 2)
        Ks, _ = sp.gains(hz[lo:hi], Q[lo:hi], R[lo:hi], F[lo:hi])
        for j in range(hi - lo):
            assert np.array_equal(Ks[j], K[lo + j])
        sp.close()
    for p_ in (plan, pp):
        p_.close()
    for h in handles:
        h.close()


def test_mixed_batch_closed_loop_matches_dropin():
    from autompc_amd.costs.terms import cost_terms
    from autompc_amd.trajectory import Trajectory
    B, T = 16, 40
    s, models, hist, hz, Q, R, F = _mixed_batch(B, 5)
    sur = seeded_mlp(s, [32], "tanh", 71)
    handles = [_handle(m) for m in models]
    hs = _lib.Handle(0, "f64")
    sur.stage_into(hs)
    goal = np.random.default_rng(6).uniform(-0.3, 0.3, size=(B, 6))
    x0 = np.random.default_rng(8).uniform(-0.5, 0.5, size=6)
    t0 = zeros(s, 1)
    t0[0].obs[:] = x0
    tasks = []
    for i in range(B):
        t = Task(s)
        t.set_cost(QuadCost(s, Q[i], R[i], F[i], goal=goal[i]))
        t.set_ctrl_bounds(-np.ones(2), np.ones(2))
        tasks.append(t)

    def run(order):
        plan = _lib.LqrPlan([handles[hist[i]] for i in order], 6, 2)
        _, st = plan.gains(hz[order], Q[order], R[order], F[order])
        assert np.all(st == 0)
        plan.set_loop(np.ones(len(order)), goal[order], -np.ones(2), np.ones(2))
        states = [models[hist[i]].traj_to_state(t0) for i in order]
        o, c = plan.closed_loop(hs, states, np.tile(x0, (len(order), 1)), T)
        plan.close()
        return o, c

    obs, ctl = run(np.arange(B))
    perm = np.random.default_rng(9).permutation(B)
    op, cp = run(perm)
    assert np.array_equal(op, obs[perm]) and np.array_equal(cp, ctl[perm])
    for i in range(B):
        ctl_i = LQR(s, tasks[i], models[hist[i]], "true", int(hz[i]))
        traj = simulate(ctl_i, x0, sim_model=sur, max_steps=T, silent=True)
        assert np.abs(traj.obs - obs[i]).max() / np.abs(traj.obs).max() < TRAJ_TOL, i
        assert np.abs(traj.ctrls - ctl[i]).max() / np.abs(traj.ctrls).max() < TRAJ_TOL, i
        # the scored loop of this problem alone: task.get_cost()(traj) of its own trajectory
        one = _lib.LqrPlan([handles[hist[i]]], 6, 2)
        one.gains(hz[i:i + 1], Q[i:i + 1], R[i:i + 1], F[i:i + 1])
        one.set_loop([1], goal[i:i + 1], -np.ones(2), np.ones(2))
        sc, o1, c1 = one.closed_loop(hs, [models[hist[i]].traj_to_state(t0)], x0[None], T,
                                     terms=cost_terms(tasks[i].get_cost(), 6, 2))
        one.close()
        assert np.array_equal(o1[0], obs[i]) and np.array_equal(c1[0], ctl[i])
        ref = tasks[i].get_cost()(Trajectory(s, T + 1, obs[i].copy(), ctl[i].copy()))
        assert abs(sc[0] - ref) <= 1e-12 * abs(ref), i
    for h in handles + [hs]:
        h.close()


def test_scored_closed_loop_matches_golden_cost():
    from autompc_amd.costs.terms import cost_terms
    from autompc_amd.trajectory import Trajectory
    g, s, m, _ = _dropin_case("arx2_small")
    t = task_of(g, s)
    hz = [int(v) for v in g["horizons"]]
    hm = _handle(m)
    plan = _lib.LqrPlan([hm] * len(hz), 4, 1)
    _, st = plan.gains(hz, g["Q"], g["R"], g["F"])
    assert np.all(st == 0)
    plan.set_loop(np.ones(len(hz)), g["goal"], g["umin"], g["umax"])
    t0 = zeros(s, 1)
    t0[0].obs[:] = g["init_obs"]
    T = g["obs_%d" % hz[0]].shape[0] - 1
    sc, obs, ctl = plan.closed_loop(hm, [m.traj_to_state(t0)] * len(hz), np.tile(m.traj_to_state(t0), (len(hz), 1)),
                                    T, terms=cost_terms(t.get_cost(), 4, 1))
    for j, h in enumerate(hz):
        ref = t.get_cost()(Trajectory(s, T + 1, g["obs_%d" % h].copy(), g["ctrls_%d" % h].copy()))
        assert abs(sc[j] - ref) <= 1e-8 * abs(ref), h
        assert np.abs(obs[j] - g["obs_%d" % h]).max() / np.abs(g["obs_%d" % h]).max() < TRAJ_TOL
    plan.close()
    hm.close()
