"""Infinite-horizon LQR without a GPU: the host Riccati iteration against the reference's goldens
(tests/golden/gen_golden_lqr_inf.py), the cap, the opt-in keyword and its defaults."""
import os

import numpy as np
import pytest

from autompc_amd import ARX, Koopman, QuadCost, System, Task
from autompc_amd.control import LQR, InfiniteHorizonLQR, LQRFactory
from autompc_amd.control import lqr as lqr_mod
from autompc_amd.control.lqr import RiccatiNotConverged, lqr_gain_inf_host
from autompc_amd.tuning.lqr_eval import LqrCandidateEvaluator

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = [("arx2", 4, 1), ("koop_mlp", 4, 1), ("arx4_mlp", 17, 6), ("arx10_wide", 17, 6)]
GAIN_TOL = 1e-12          # of max|K|: what the finite-horizon gains are held to (test_gpu_lqr.py)
MARGIN = 1e-6             # the fixtures' dP sequences keep this distance from the threshold


def gold(name):
    return np.load(os.path.join(GOLD, "lqrinf_%s.npz" % name))


def system(no, nu):
    return System(["x%d" % i for i in range(no)], ["u%d" % i for i in range(nu)], dt=0.05)


def model_of(name, g, no, nu):
    s = system(no, nu)
    if name == "koop_mlp":
        m = Koopman(s, method="lstsq", poly_basis=True, poly_degree=int(g["poly_degree"]))
        m.set_parameters({"A": g["A"], "B": g["B"]})
    else:
        m = ARX(s, history=int(g["history"]))
        m.set_parameters({"coeffs": g["coeffs"]})
    return s, m


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


@pytest.mark.parametrize("name,no,nu", CASES)
def test_host_gain_matches_reference(name, no, nu):
    g = gold(name)
    dP, thr = g["dP"], float(g["threshold"])
    assert len(dP) == int(g["iters"])
    assert np.all(dP[:-1] > thr * (1 + MARGIN)) and dP[-1] < thr * (1 - MARGIN)
    _, m = model_of(name, g, no, nu)
    A, B = m.to_linear()
    K, iters = lqr_gain_inf_host(A, B, g["Q"], g["R"], threshold=thr)
    assert iters == int(g["iters"])
    assert np.abs(K - g["K"]).max() <= GAIN_TOL * np.abs(g["K"]).max()


def test_cap_raises_not_converged():
    A, B, Q, R = bias_system()
    with pytest.raises(RiccatiNotConverged, match="max_iter = 200"):
        lqr_gain_inf_host(A, B, Q, R, max_iter=200)
    assert issubclass(RiccatiNotConverged, np.linalg.LinAlgError)
    # without the bias the same system converges well inside the cap
    A0, B0, _, _ = bias_system(bias=0.0)
    K, iters = lqr_gain_inf_host(A0, B0, Q, R, max_iter=200)
    assert iters < 200 and np.all(np.isfinite(K))
    # converging exactly at the cap is converged
    K2, iters2 = lqr_gain_inf_host(A0, B0, Q, R, max_iter=iters)
    assert iters2 == iters and np.array_equal(K, K2)
    with pytest.raises(RiccatiNotConverged):
        lqr_gain_inf_host(A0, B0, Q, R, max_iter=iters - 1)


def test_bad_parameters_refused():
    A, B, Q, R = bias_system(bias=0.0)
    for thr in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(ValueError, match="threshold"):
            lqr_gain_inf_host(A, B, Q, R, threshold=thr)
    for mi in (0, lqr_mod.INF_MAX_ITER_LIMIT + 1):
        with pytest.raises(ValueError, match="max_iter"):
            lqr_gain_inf_host(A, B, Q, R, max_iter=mi)


def _task(s):
    t = Task(s)
    t.set_cost(QuadCost(s, np.eye(s.obs_dim), np.eye(s.ctrl_dim), np.eye(s.obs_dim)))
    return t


def test_defaults_still_refuse():
    s = system(4, 1)
    arx = ARX(s, history=2)
    with pytest.raises(NotImplementedError, match="dare"):
        LQR(s, _task(s), arx, "false")
    with pytest.raises(NotImplementedError, match="dare"):
        InfiniteHorizonLQR(s, _task(s), arx)
    with pytest.raises(NotImplementedError, match="dare"):
        LQR(s, _task(s), arx, "false", infinite_horizon="refuse")
    ev = LqrCandidateEvaluator(s, _task(s), model=arx)
    assert ev.infinite_horizon == "refuse"
    assert lqr_mod.INF_THRESHOLD_DEFAULT == 1e-3 and lqr_mod.INF_MAX_ITER_DEFAULT == 10000


def test_keyword_is_spelled_the_same_everywhere():
    s = system(4, 1)
    arx = ARX(s, history=2)
    assert lqr_mod.INFINITE_HORIZON_CHOICES == ("refuse", "iterate")
    for bad in ("yes", True, None, "Iterate"):
        with pytest.raises(ValueError, match="infinite_horizon"):
            LQR(s, _task(s), arx, "false", infinite_horizon=bad)
        with pytest.raises(ValueError, match="infinite_horizon"):
            LQR(s, _task(s), arx, "true", 10, infinite_horizon=bad)       # refused before anything runs
        with pytest.raises(ValueError, match="infinite_horizon"):
            InfiniteHorizonLQR(s, _task(s), arx, infinite_horizon=bad)
        with pytest.raises(ValueError, match="infinite_horizon"):
            LqrCandidateEvaluator(s, _task(s), model=arx, infinite_horizon=bad)
    ev = LqrCandidateEvaluator(s, _task(s), model=arx, infinite_horizon="iterate", inf_threshold=1e-4, inf_max_iter=50)
    assert (ev.infinite_horizon, ev.inf_threshold, ev.inf_max_iter) == ("iterate", 1e-4, 50)
    with pytest.raises(ValueError, match="max_iter"):
        LqrCandidateEvaluator(s, _task(s), model=arx, infinite_horizon="iterate", inf_max_iter=0)
    # the factory's keyword merge hands the keyword to LQR
    f = LQRFactory(s, infinite_horizon="iterate", max_iter=77)
    assert f.kwargs == {"infinite_horizon": "iterate", "max_iter": 77}


def test_host_controller_run_is_the_references():
    """InfiniteHorizonLQR.run (lqr.py:126-136) around a host gain: u = K modelstate, no goal, no clip -- the first
    control of the reference's closed loop, which lies outside the task's bounds."""
    from autompc_amd import zeros
    from autompc_amd.tuning.lqr_eval import _HostInfiniteHorizonLQR
    g = gold("arx2")
    s, m = model_of("arx2", g, 4, 1)
    t = Task(s)
    t.set_cost(QuadCost(s, g["Q"], g["R"], np.eye(4), goal=g["goal"]))
    t.set_ctrl_bounds(g["umin"], g["umax"])
    ctl = _HostInfiniteHorizonLQR(s, t, m, "iterate")
    assert ctl.iters == int(g["iters"]) and ctl.state_dim == m.state_dim + 1
    t0 = zeros(s, 1)
    t0[0].obs[:] = g["init_obs"]
    state = ctl.traj_to_state(t0)
    np.testing.assert_allclose(state, g["cstate0"], rtol=0, atol=1e-14)
    u, new = ctl.run(state, g["init_obs"])
    assert np.array_equal(new[-1:], u) and new.shape == state.shape
    assert np.abs(u - g["ctrls"][0]).max() <= 1e-10 * np.abs(g["ctrls"][0]).max()
    assert np.abs(g["ctrls"][0]).max() > g["umax"].max()          # the bound was not applied
