"""Layer 0's bias through the spare K column (TileNet::BIAS0_IN_K, csrc/mlp_tile.hpp): the shape-specialised
16-row f64 rollout tile keeps 1.0 in the last pad column of [x | u | 0] and the bias in the matching row of the
resident layer-0 fragments, so the bias is the last link of the MFMA's k-ordered fma chain, fma(b, 1, acc) =
RN(acc + b), and the epilogue has no add.  The run-time-shape kernels keep the separate add: both must give the
same bits, and both must agree with the oracle rollout.  Needs MI355X."""
import numpy as np
import pytest

from helpers import make_system, rel_err
from oracle import mlp as omlp
from oracle.costs import QuadCostOracle
from oracle.mlp import MLPOracle
from oracle.mppi import MPPIOracle

pytestmark = pytest.mark.gpu

# registered shapes (csrc/shapes.hpp).  17 + 6 = 23 of 24: one pad column (eight-wave tiles, bias per register);
# 4 + 1 = 5 of 8: three pad columns, four-wave tile (the other layers' biases from LDS); 2 + 1 = 3 of 8: five
SHAPES = [
    (17, 6, [256, 256], "relu"),
    (17, 6, [256, 256], "tanh"),
    (17, 6, [128, 128], "relu"),
    (4, 1, [64, 64], "relu"),
    (2, 1, [64, 64], "relu"),
]
# (N, H) of the three problems of the plan: a tile with 15 rows past N, a full tile, a second tile with one live row
PROBLEMS = ((1, 2), (16, 3), (17, 2))
BOUNDS = (-0.7, 0.9)
SIGMA, LMDA = (1.0, 0.6, 0.8), (1.0, 0.4, 0.7)


def _setup(nx, nu, hidden, act, seed=11):
    p = omlp.random_params(nx, nu, hidden, act, seed=seed)
    rng = np.random.default_rng(seed + 1)
    Q, R, F = np.diag(rng.uniform(0.5, 2, nx)), np.diag(rng.uniform(0.01, 0.1, nu)), np.diag(rng.uniform(0.5, 2, nx))
    goal = rng.normal(scale=0.1, size=nx)
    return p, (Q, R, F, goal)


def _inputs(nx, nu, seed=3):
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-0.1, 0.1, size=(len(PROBLEMS), nx))
    acts = [rng.normal(size=(H, nu)) for _, H in PROBLEMS]
    eps = [rng.normal(size=(N, H, nu)) for N, H in PROBLEMS]
    return x0, acts, eps


def _solve_twice(static, nx, nu, act, p, cost, x0, acts, eps, monkeypatch):
    """(kernel kind, costs of the first solve, [act_seq, u, costs, eps_out] after the second) on 16-row tiles.
    The second solve starts from the first one's warm start."""
    from autompc_amd import _lib
    monkeypatch.setenv("AMPC_STATIC", static)
    h = _lib.Handle(0, "f64")
    h.set_mlp(nx, nu, p["weights"], p["biases"], act, p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"])
    h.set_quad_costs(*cost)
    h.set_ctrl_bounds(np.full(nu, BOUNDS[0]), np.full(nu, BOUNDS[1]))
    plan = _lib.MppiPlan(h, [N for N, _ in PROBLEMS], [H for _, H in PROBLEMS], list(SIGMA), list(LMDA))
    plan.set_geometry(16, 0)
    plan.upload(x0=x0, act_seq=np.concatenate([a.ravel() for a in acts]), eps=np.concatenate([e.ravel() for e in eps]))
    plan.solve()
    kind = plan.kernel_kind()
    first = plan.download(act_seq=False, u=False, costs=True)[2].copy()
    plan.solve()
    out = plan.download(costs=True, eps_out=True)
    plan.close()
    h.close()
    return kind, first, out


def _both(nx, nu, act, p, cost, x0, acts, eps, monkeypatch):
    s = _solve_twice("1", nx, nu, act, p, cost, x0, acts, eps, monkeypatch)
    g = _solve_twice("0", nx, nu, act, p, cost, x0, acts, eps, monkeypatch)
    assert s[0] == 1, "the plan did not pick the shape-specialised kernels"
    assert g[0] == 0
    return s, g


def _assert_same_bits(s, g):
    np.testing.assert_array_equal(s[1], g[1])
    for a, b in zip(s[2], g[2]):            # act_seq, u, costs, eps_out
        np.testing.assert_array_equal(a, b)


def _oracle_costs(nx, nu, p, cost, b, x0, acts, eps):
    Q, R, F, goal = cost
    N, H = PROBLEMS[b]
    orc = MPPIOracle(MLPOracle(make_system(nx, nu), p), QuadCostOracle(Q, R, F, goal), np.tile(np.array(BOUNDS), (nu, 1)),
                     horizon=H, num_path=N, sigma=SIGMA[b], lmda=LMDA[b])
    orc.act_sequence = acts[b].copy()
    return orc.do_rollouts(x0[b], eps[b].copy())[0]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%dx%d_%s" % (s[0], s[1], len(s[2]), s[2][0], s[3]))
def test_bias_column_has_the_bits_of_the_separate_add(shape, monkeypatch):
    nx, nu, hidden, act = shape
    p, cost = _setup(nx, nu, hidden, act)
    x0, acts, eps = _inputs(nx, nu)
    s, g = _both(nx, nu, act, p, cost, x0, acts, eps, monkeypatch)
    _assert_same_bits(s, g)
    assert np.all(np.isfinite(s[2][2]))
    # a bias that is wrong in code both kernels share would pass the comparison above
    off = 0
    for b, (N, _) in enumerate(PROBLEMS):
        ref = _oracle_costs(nx, nu, p, cost, b, x0, acts, eps)
        err = rel_err(s[1][off:off + N], ref)
        print("problem %d: cost rel err %.3e" % (b, err))
        assert err < 1e-9
        off += N


@pytest.mark.parametrize("stress", ["zero_weights", "bias_1e8", "bias_1e-8"])
def test_bias_magnitudes_against_the_accumulated_sum(stress, monkeypatch):
    """The last link of the chain at its extremes: the bias alone (every product before it is zero), a bias that
    swamps the sum and one that the sum swamps -- RN(acc + b) either way, the bits of the separate add."""
    nx, nu, hidden, act = SHAPES[0]
    p, cost = _setup(nx, nu, hidden, act)
    p["weights"] = [w.copy() for w in p["weights"]]
    p["biases"] = [b.copy() for b in p["biases"]]
    if stress == "zero_weights":
        p["weights"][0][...] = 0.0
        assert np.all(p["biases"][0] != 0.0)
    else:
        p["biases"][0] *= float(stress.split("_")[1])
    x0, acts, eps = _inputs(nx, nu)
    s, g = _both(nx, nu, act, p, cost, x0, acts, eps, monkeypatch)
    _assert_same_bits(s, g)
    assert np.all(np.isfinite(s[2][2]))


@pytest.mark.parametrize("where", ["noise", "x0"])
def test_the_constant_column_neither_masks_nor_spreads_a_nan(where, monkeypatch):
    nx, nu, hidden, act = SHAPES[0]
    p, cost = _setup(nx, nu, hidden, act)
    x0, acts, eps = _inputs(nx, nu)
    if where == "noise":
        eps[2][5, 0, 2] = np.nan           # one sample of the third problem's first tile
    else:
        x0[1, 3] = np.nan                  # every sample of the second problem
    s, g = _both(nx, nu, act, p, cost, x0, acts, eps, monkeypatch)
    np.testing.assert_array_equal(np.isfinite(s[1]), np.isfinite(g[1]))
    np.testing.assert_array_equal(np.isfinite(s[2][2]), np.isfinite(g[2][2]))
    _assert_same_bits(s, g)
    bad = np.zeros(sum(N for N, _ in PROBLEMS), dtype=bool)
    if where == "noise":
        bad[1 + 16 + 5] = True
    else:
        bad[1:17] = True
    np.testing.assert_array_equal(~np.isfinite(s[1]), bad)
