"""LQR controller surface without a GPU: LQRFactory's space, the refusals, the tuning-configuration keys; the host
gain and the numpy model of the gain kernel at the edge cases (lqr_edge_cases.py) against long double."""
import numpy as np
import pytest

from autompc_amd import MLP, QuadCost, System, Task
from autompc_amd.control import LQR, LQRFactory, FiniteHorizonLQR, InfiniteHorizonLQR
from autompc_amd.control import lqr as lqr_mod
from autompc_amd.sysid import ARX
from autompc_amd.tuning.configs import candidate_from_config, sample_pipeline_configs
import lqr_edge_cases as E


def _system(no=4, nu=1):
    return System(["x%d" % i for i in range(no)], ["u%d" % i for i in range(nu)], dt=0.05)


def _task(s, obs_bounded=False):
    t = Task(s)
    t.set_cost(QuadCost(s, np.eye(s.obs_dim), np.eye(s.ctrl_dim), np.eye(s.obs_dim)))
    if obs_bounded:
        t.set_obs_bounds(-np.ones(s.obs_dim), np.ones(s.obs_dim))
    return t


def test_factory_space_constants():
    # lqr.py:214-224
    assert lqr_mod.FINITE_HORIZON_CHOICES == ("true", "false")
    assert lqr_mod.HORIZON_RANGE == (1, 1000) and lqr_mod.HORIZON_DEFAULT == 10
    assert LQRFactory.name == "LQR" and LQRFactory.Controller is LQR


def test_is_compatible():
    s = _system()
    arx = ARX(s, history=2)
    mlp = MLP(s, n_hidden_layers=1, hidden_size=8)
    assert LQR.is_compatible(s, _task(s), arx)
    assert FiniteHorizonLQR.is_compatible(s, _task(s), arx)
    assert not LQR.is_compatible(s, _task(s), mlp)
    assert not LQR.is_compatible(s, _task(s, obs_bounded=True), arx)


def test_refusals():
    s = _system()
    with pytest.raises(TypeError, match="linear model"):
        LQR(s, _task(s), MLP(s, n_hidden_layers=1, hidden_size=8), "true", 10)
    with pytest.raises(NotImplementedError, match="dare"):
        LQR(s, _task(s), ARX(s, history=2), "false")
    with pytest.raises(NotImplementedError):
        InfiniteHorizonLQR(s, _task(s), ARX(s, history=2))


def test_lqr_configs_refused_by_the_tuning_layer():
    # no batched evaluator scores LQR candidates yet: an LQRFactory configuration must not fall through to the
    # iLQR mapping (same horizon key) and be scored as an iLQR candidate
    s = _system(3, 2)
    for finite in ("true", "false"):
        with pytest.raises(NotImplementedError, match="finite_horizon"):
            candidate_from_config(s, {"_ctrlr:finite_horizon": finite, "_ctrlr:horizon": 250, "_cost:x0_Q": 1.0})
    with pytest.raises(ValueError):
        sample_pipeline_configs(s, 1, np.random.default_rng(0), controller="lqr")


def test_horizon_outside_factory_range_refused():
    s = _system()
    for h in (0, 1001):
        with pytest.raises(ValueError, match="1..1000"):
            LQR(s, _task(s), ARX(s, history=2), "true", h)


@pytest.mark.parametrize("name", list(E.CASES))
def test_host_gain_against_long_double(name):
    """lqr_gain_host at the edge cases (tile edges, non-symmetric Q / F / R, pivoting R) against the long-double
    recursion of tests/golden/lqr_edges.npz."""
    arrays = E.make_case(name)
    fx = E.fixture()
    np.testing.assert_array_equal(E.checksum(arrays), fx["checksum_" + name])
    K = lqr_mod.lqr_gain_host(*arrays, E.CASES[name]["horizon"])
    assert E.rel_err(K, fx["K_" + name]) <= 1e-13


@pytest.mark.parametrize("name", list(E.CASES))
def test_kernel_model_against_long_double(name):
    """The numpy model of lqr_gains_kernel's arithmetic (lqr_edge_cases.kernel_model): within the device's own
    tolerance of the long-double gain on every cost kind, and the row exchanges the fixture recorded -- one or more in
    every solve of a pivoting case, none anywhere else."""
    arrays = E.make_case(name)
    fx = E.fixture()
    np.testing.assert_array_equal(E.checksum(arrays), fx["checksum_" + name])
    K, status, counts = E.kernel_model(*arrays, E.CASES[name]["horizon"])
    assert status == 0
    assert E.rel_err(K, fx["K_" + name]) <= E.tolerance(fx["host_err_" + name])
    np.testing.assert_array_equal(counts, fx["exchanges_" + name])
    assert min(counts) >= 1 if E.pivoting(name) else max(counts) == 0


def test_kernel_model_singular():
    A, B, Q, R, F = E.make_case("n17_u16_o17_diag")
    Rs = np.diag(np.arange(1.0, 17.0))
    Rs[7, 7] = 0.0
    K, status, _ = E.kernel_model(A, B, 0 * Q, Rs, 0 * F, 2)
    assert status == 1 and np.all(np.isnan(K))


def test_mppi_and_ilqr_configs_unchanged():
    s = _system(3, 2)
    ilqr = candidate_from_config(s, {"_ctrlr:horizon": 12, "_cost:x0_Q": 1.0, "_cost:x1_Q": 1.0, "_cost:x2_Q": 1.0,
                                  "_cost:x0_F": 1.0, "_cost:x1_F": 1.0, "_cost:x2_F": 1.0, "_cost:u0_R": 1.0,
                                  "_cost:u1_R": 1.0})
    assert ilqr.get("controller") != "lqr" and ilqr["horizon"] == 12 and "num_path" not in ilqr

