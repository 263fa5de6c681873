"""mppi_combine_kernel (csrc/mppi_kernels.hpp) requests everything it reads before its first reduction and adds the
normaliser in the same pass as the nu weighted sums.  Every sum keeps its order -- per thread the tiles i = tid,
tid + 256, ..; per wave the shuffle tree; across waves w = 0 .. 3 -- so the update must agree with the oracle as
before, repeat bit for bit, skip a dead tile, and leave the noise-ahead blocks of the same launch alone.
Needs MI355X."""
import numpy as np
import pytest

from helpers import make_system, rel_err
from oracle import mlp as omlp
from oracle.costs import QuadCostOracle
from oracle.mlp import MLPOracle
from oracle.mppi import MPPIOracle

pytestmark = pytest.mark.gpu

NX, NU, HIDDEN, ACT = 17, 6, [256, 256], "relu"
H = 2
SIGMA, LMDA = (1.0, 0.5), (1.0, 0.4)


def _params():
    return omlp.random_params(NX, NU, HIDDEN, ACT, seed=7)


def _handle(p, Q, R, F, goal, lo, hi):
    from autompc_amd import _lib
    h = _lib.Handle(0, "f64")
    h.set_mlp(NX, NU, p["weights"], p["biases"], ACT, p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"])
    h.set_quad_costs(Q, R, F, goal)
    h.set_ctrl_bounds(np.full(NU, lo), np.full(NU, hi))
    return h


def _oracle(p, Q, R, F, goal, bounds, N, Hh, sigma, lmda, x0, act0, eps):
    orc = MPPIOracle(MLPOracle(make_system(NX, NU), p), QuadCostOracle(Q, R, F, goal), np.tile(np.array(bounds), (NU, 1)),
                     horizon=Hh, num_path=N, sigma=sigma, lmda=lmda)
    orc.act_sequence = act0.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        u, _ = orc.run(np.concatenate([x0, np.zeros(NU)]), x0, eps_nhu=eps.copy())
    return u, orc.act_sequence.copy(), orc.last_costs.copy()


# tiles per problem: one, two, more than a wave's worth of one thread each, and one more than the block is wide
# (thread 0 takes tiles 0 and 256)
@pytest.mark.parametrize("N", [16, 32, 272, 4112], ids=lambda n: "tiles%d" % (n // 16))
def test_update_agrees_with_the_oracle_and_repeats(N):
    from autompc_amd import _lib
    p = _params()
    rng = np.random.default_rng(N)
    Q, R, F = np.diag(rng.uniform(0.5, 2, NX)), np.diag(rng.uniform(0.01, 0.1, NU)), np.diag(rng.uniform(0.5, 2, NX))
    goal = rng.normal(scale=0.1, size=NX)
    x0 = rng.uniform(-0.1, 0.1, size=(2, NX))
    acts = [rng.normal(scale=0.3, size=(H, NU)) for _ in range(2)]
    eps = [rng.normal(scale=np.sqrt(SIGMA[b]), size=(N, H, NU)) for b in range(2)]
    got = []
    for _ in range(2):
        h = _handle(p, Q, R, F, goal, -1.0, 1.0)
        plan = _lib.MppiPlan(h, [N, N], [H, H], list(SIGMA), list(LMDA))
        plan.set_geometry(16, 0)
        assert plan.info()["samples_per_wg"] == 16
        plan.upload(x0=x0, act_seq=np.concatenate([a.ravel() for a in acts]), eps=np.concatenate([e.ravel() for e in eps]))
        plan.solve()
        got.append(plan.download(costs=True))
        plan.close()
        h.close()
    for a, b in zip(got[0][:3], got[1][:3]):          # act_seq, u, costs
        np.testing.assert_array_equal(a, b)
    a_all, u_all, c_all, _ = got[0]
    for b in range(2):
        u, a, c = _oracle(p, Q, R, F, goal, (-1.0, 1.0), N, H, SIGMA[b], LMDA[b], x0[b], acts[b], eps[b])
        errs = (rel_err(c_all[b * N:(b + 1) * N], c), rel_err(a_all[b * H * NU:(b + 1) * H * NU].reshape(H, NU), a),
                rel_err(u_all[b], u))
        print("N %d problem %d: costs %.3e act_seq %.3e u %.3e" % ((N, b) + errs))
        assert errs[0] < 1e-9 and errs[1] < 1e-8 and errs[2] < 1e-8


def test_a_dead_tile_is_skipped():
    """A tile whose every cost is +inf publishes zero sums; the combine kernel loads them with the others now and
    must still give them weight 0 (the construction of test_fused_update_with_an_all_inf_tile_matches_the_plain_update)."""
    from autompc_amd import _lib
    N, Hh = 96, 6
    p = omlp.random_params(NX, NU, HIDDEN, ACT, seed=3)
    Q, R, F = 1e300 * np.eye(NX), 0.01 * np.eye(NU), np.eye(NX)
    rng = np.random.default_rng(0)
    eps = 1e-6 * rng.normal(size=(N, Hh, NU))
    eps[32:48] = np.sign(rng.normal(size=(16, Hh, NU)))       # the third tile saturates at +-1e6: its costs overflow
    act0 = 1e-6 * rng.normal(size=(Hh, NU))
    x0 = rng.uniform(-0.1, 0.1, size=NX)
    h = _handle(p, Q, R, F, np.zeros(NX), -1e6, 1e6)
    plan = _lib.MppiPlan(h, [N], [Hh], [1.0], [1.0])
    plan.set_geometry(16, 0)
    plan.upload(x0=x0, act_seq=act0, eps=eps)
    plan.solve()
    a, u, costs, _ = plan.download(costs=True)
    plan.close()
    h.close()
    assert np.all(np.isinf(costs[32:48])) and np.all(np.isfinite(np.delete(costs, np.s_[32:48])))
    uo, ao, co = _oracle(p, Q, R, F, np.zeros(NX), (-1e6, 1e6), N, Hh, 1.0, 1.0, x0, act0, eps)
    assert np.all(np.isinf(co[32:48])) and np.all(np.isfinite(ao))
    live = np.isfinite(co)
    errs = (rel_err(costs[live], co[live]), rel_err(a.reshape(Hh, NU), ao), rel_err(u[0], uo))
    print("dead tile: costs %.3e act_seq %.3e u %.3e" % errs)
    assert errs[0] < 1e-9 and errs[1] < 1e-8 and errs[2] < 1e-8


def test_noise_ahead_of_three_consecutive_streams_is_the_generators(monkeypatch):
    """Blocks x >= max_h of the combine launch form the next stream index's noise; three indices in a row against
    a generator launch each."""
    from autompc_amd import _lib
    p = _params()
    rng = np.random.default_rng(1)
    x0 = rng.uniform(-0.1, 0.1, size=(2, NX))
    N = 272

    def run(ahead):
        monkeypatch.setenv("AMPC_NOISE_AHEAD", ahead)
        h = _handle(p, np.eye(NX), 0.01 * np.eye(NU), np.eye(NX), np.zeros(NX), -1.0, 1.0)
        plan = _lib.MppiPlan(h, [N, N], [H, H], [0.09, 0.04], [1.0, 0.5])
        plan.set_geometry(16, 0)
        plan.upload(x0, np.zeros(2 * H * NU))
        out = []
        for s in (5, 6, 7):
            plan.generate_eps(77, s)
            plan.solve()
            a, u, _, e = plan.download(eps_out=True)
            out.append((a.copy(), u.copy(), e.copy()))
        plan.close()
        h.close()
        return out
    a, b = run("1"), run("0")
    for i, (x, y) in enumerate(zip(a, b)):
        for k in range(3):
            assert np.array_equal(x[k], y[k]), (i, k)
    assert not np.array_equal(a[0][2], a[1][2])       # (the streams differ: the comparison is not vacuous)
