"""The pinned 16-row f64 rollout tile computes layer 0 and the hidden layers TRANSPOSED and hands a wave's
activations from MFMA accumulator registers to its next MFMAs (TileNet::CHAIN, csrc/mlp_tile.hpp): a sample
is an MFMA column there, a hidden unit a row.  Every output element is still the same k-ordered chain of the
same products, so the shape-specialised kernels must give the bits of the run-time-shape kernels (which are
not transposed), and both must agree with the oracle rollout.  Needs MI355X."""
import numpy as np
import pytest

from helpers import make_system, rel_err
from oracle import mlp as omlp
from oracle.costs import QuadCostOracle
from oracle.mlp import MLPOracle
from oracle.mppi import MPPIOracle

pytestmark = pytest.mark.gpu

# registered shapes (csrc/shapes.hpp): 2 x 256 is the own-group-first tile with the 4x4x4 output tail
# (8 waves x 2 column tiles), 2 x 128 the tile without own-group chaining (8 waves x 1 column tile), 2 x 64 the
# four-wave tile, which takes the transposed epilogue's biases from LDS
REGISTERED = [
    (17, 6, [256, 256], "relu"),
    (17, 6, [256, 256], "tanh"),
    (17, 6, [128, 128], "relu"),
    (4, 1, [64, 64], "relu"),
]
# (N, H) of the two problems of a plan.  Sample counts 1 / 16 / 17 / 300: a tile with 15 rows past N, a full
# tile, a second tile with one live row, many tiles with a ragged end.  Horizons 2 / 3 / 12: one loop carry,
# two, several (a horizon of 1 is no MPPI problem: see test_a_horizon_of_one_is_refused).
PROBLEMS = [
    ((300, 12), (1, 2)),
    ((17, 2), (16, 12)),
    ((16, 12), (17, 3)),
    ((1, 3), (300, 2)),
]
BOUNDS = (-0.7, 0.9)
SIGMA, LMDA = (1.0, 0.6), (1.0, 0.4)


def _setup(nx, nu, hidden, act, seed=11):
    p = omlp.random_params(nx, nu, hidden, act, seed=seed)
    rng = np.random.default_rng(seed + 1)
    Q, R, F = np.diag(rng.uniform(0.5, 2, nx)), np.diag(rng.uniform(0.01, 0.1, nu)), np.diag(rng.uniform(0.5, 2, nx))
    goal = rng.normal(scale=0.1, size=nx)
    return p, (Q, R, F, goal)


def _handle(nx, nu, act, p, cost):
    from autompc_amd import _lib
    h = _lib.Handle(0, "f64")
    h.set_mlp(nx, nu, p["weights"], p["biases"], act, p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"])
    h.set_quad_costs(*cost)
    h.set_ctrl_bounds(np.full(nu, BOUNDS[0]), np.full(nu, BOUNDS[1]))
    return h


def _inputs(nx, nu, problems, seed=3):
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-0.1, 0.1, size=(len(problems), nx))
    acts = [rng.normal(size=(H, nu)) for _, H in problems]
    eps = [rng.normal(size=(N, H, nu)) for N, H in problems]
    return x0, acts, eps


def _solve_twice(h, problems, x0, acts, eps):
    """(kernel kind, first problem's costs of the first solve, everything after the second solve) on 16-row
    tiles.  The second solve starts from the first one's warm start and clipped noise."""
    from autompc_amd import _lib
    plan = _lib.MppiPlan(h, [N for N, _ in problems], [H for _, H in problems], list(SIGMA), list(LMDA))
    plan.set_geometry(16, 0)        # the 16-row tile (rules out the taller tiles and the four-row kernel)
    plan.upload(x0=x0, act_seq=np.concatenate([a.ravel() for a in acts]), eps=np.concatenate([e.ravel() for e in eps]))
    plan.solve()
    kind = plan.kernel_kind()
    first = plan.download(act_seq=False, u=False, costs=True)[2][:problems[0][0]].copy()
    plan.solve()
    out = plan.download(costs=True, eps_out=True)      # act_seq, u, costs, eps_out
    plan.close()
    return kind, first, out


def _oracle_costs(nx, nu, p, cost, N, H, x0, act0, eps):
    Q, R, F, goal = cost
    orc = MPPIOracle(MLPOracle(make_system(nx, nu), p), QuadCostOracle(Q, R, F, goal), np.tile(np.array(BOUNDS), (nu, 1)),
                     horizon=H, num_path=N, sigma=SIGMA[0], lmda=LMDA[0])
    orc.act_sequence = act0.copy()
    return orc.do_rollouts(x0, eps.copy())[0]


def _static_and_general(nx, nu, act, p, cost, problems, x0, acts, eps, monkeypatch):
    got = {}
    for static in ("1", "0"):
        monkeypatch.setenv("AMPC_STATIC", static)
        h = _handle(nx, nu, act, p, cost)
        got[static] = _solve_twice(h, problems, x0, acts, eps)
        h.close()
    assert got["1"][0] == 1, "the plan did not pick the shape-specialised kernels"
    assert got["0"][0] == 0
    return got["1"], got["0"]


@pytest.mark.parametrize("problems", PROBLEMS, ids=lambda pr: "N%d_H%d-N%d_H%d" % (pr[0] + pr[1]))
@pytest.mark.parametrize("shape", REGISTERED, ids=lambda s: "%dx%d_%s" % (len(s[2]), s[2][0], s[3]))
def test_chained_kernel_has_the_bits_of_the_general_kernel(shape, problems, monkeypatch):
    nx, nu, hidden, act = shape
    p, cost = _setup(nx, nu, hidden, act)
    x0, acts, eps = _inputs(nx, nu, problems)
    (_, first_s, out_s), (_, first_g, out_g) = _static_and_general(nx, nu, act, p, cost, problems, x0, acts, eps,
                                                                   monkeypatch)
    np.testing.assert_array_equal(first_s, first_g)
    for a, b in zip(out_s, out_g):          # act_seq, u, costs, eps_out
        np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(out_s[2]))
    # a transposition that is wrong in code both kernels share would pass the comparison above
    (N, H) = problems[0]
    ref = _oracle_costs(nx, nu, p, cost, N, H, x0[0], acts[0], eps[0])
    assert rel_err(first_s, ref) < 1e-9


def test_a_nan_in_one_samples_noise_stays_in_that_sample(monkeypatch):
    """A sample is an MFMA column now: a NaN in it must not reach another sample's cost."""
    nx, nu, hidden, act = REGISTERED[1]
    problems = ((300, 12), (17, 3))
    bad = 37
    p, cost = _setup(nx, nu, hidden, act)
    x0, acts, eps = _inputs(nx, nu, problems)
    eps[0][bad, 1, 2] = np.nan
    (_, first_s, out_s), (_, first_g, out_g) = _static_and_general(nx, nu, act, p, cost, problems, x0, acts, eps,
                                                                   monkeypatch)
    assert np.isnan(first_s[bad])
    assert np.all(np.isfinite(np.delete(first_s, bad)))
    np.testing.assert_array_equal(first_s, first_g)
    for a, b in zip(out_s, out_g):
        np.testing.assert_array_equal(a, b)
    # the other problem of the plan is untouched
    assert np.all(np.isfinite(out_s[2][problems[0][0]:]))
    clean = eps[0].copy()
    clean[bad] = 0.0
    ref = _oracle_costs(nx, nu, p, cost, problems[0][0], problems[0][1], x0[0], acts[0], clean)
    assert rel_err(np.delete(first_s, bad), np.delete(ref, bad)) < 1e-9


def test_a_horizon_of_one_is_refused():
    """The reference's shift of the warm start (a[-1] = a[-2], mppi.py:120-124) needs two steps, and so does
    ampc_mppi_plan_create: there is no rollout without a loop carry to chain."""
    from autompc_amd import _lib
    nx, nu, hidden, act = REGISTERED[2]
    p, cost = _setup(nx, nu, hidden, act)
    h = _handle(nx, nu, act, p, cost)
    with pytest.raises(_lib.AmpcError):
        _lib.MppiPlan(h, [16], [1], [1.0], [1.0])
    h.close()


def test_runtime_compiled_three_layer_shape(monkeypatch):
    """What no registered shape reaches: two full output tiles and no tail (24 states), a streamed first layer
    (28 inputs), own-group chaining into a MIDDLE layer with ping-pong buffers, and a third hidden layer whose
    bias comes from LDS.  Run-time compiled kernels against the run-time-shape kernels, 16-row tiles."""
    nx, nu, hidden, act = 24, 4, [256, 256, 256], "relu"
    problems = ((300, 12), (17, 2))
    p, cost = _setup(nx, nu, hidden, act, seed=5)
    x0, acts, eps = _inputs(nx, nu, problems)
    monkeypatch.setenv("AMPC_JIT", "0")
    h = _handle(nx, nu, act, p, cost)
    assert h.jit_status()[0] == 0
    kind, first_g, out_g = _solve_twice(h, problems, x0, acts, eps)
    assert kind == 0
    h.close()
    monkeypatch.setenv("AMPC_JIT", "1")
    h = _handle(nx, nu, act, p, cost)
    h.jit_wait()
    st, msg = h.jit_status()
    assert st == 2 and msg.endswith(".so"), msg
    kind, first_s, out_s = _solve_twice(h, problems, x0, acts, eps)
    h.close()
    assert kind == 2, "the plan did not pick the run-time compiled kernels"
    np.testing.assert_array_equal(first_s, first_g)
    for a, b in zip(out_s, out_g):
        np.testing.assert_array_equal(a, b)
    ref = _oracle_costs(nx, nu, p, cost, problems[0][0], problems[0][1], x0[0], acts[0], eps[0])
    assert rel_err(first_s, ref) < 1e-9
