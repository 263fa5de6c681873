"""Hidden-layer biases in the fused MLP tile (csrc/mlp_tile.hpp), on networks whose biases DOMINATE the
pre-activations: every hidden bias is ~1e3 x the weighted sum it is added to, so a bias that a code path
drops, doubles or takes from the wrong column / layer is an O(1) error in everything downstream, not a
rounding-level one.  One MPPI solve (two ragged problems), pred_batch and pred_diff_batch per shape, against
the CPU oracle; 16 / 32 / 64-row tiles and the shape-specialised / run-time-shape kernels must give the same
bits, and the f32 mode must follow f64.  Needs MI355X.

The networks: hidden weights scaled down until a layer's weighted sums have rms 1e-3, biases N(0, 1) -- the
ratio is 1e3 and the smooth activations stay out of saturation, so their derivatives are well conditioned in
the oracle and the Jacobians can be held to 1e-10 each (jx - I and ju separately).

The same bits across tile heights:
  * pred_batch (AMPC_MT = 1 / 2 / 4): always -- a row's output is the same chain of MFMAs and the same sum
    over the waves' partials whatever the height of its tile.
  * per-sample costs of the solve: a sample's terms are added up by TPS = 64 W / rows threads (thread r owns
    state columns and controls r, r + TPS, ..; the TPS partial sums meet in an xor butterfly).  While
    max(nx, nu) <= TPS every thread owns at most one column and one control, the other lanes add zeros, and
    the sum is grouped as on 16-row tiles: those heights are compared bit for bit (costs_bitwise()).  Beyond
    that a thread adds several columns into one partial sum -- another grouping (at the commit before this
    file, nx = 17: 6 of 167 costs differ in the last bit between 16- and 32-row tiles) -- and the costs are
    held to the rounding of a sum of <= 300 non-negative terms.
  * the updated sequence: never -- every tile publishes one partial sum of its rows' weighted noise, scaled
    by its own minimum cost, so the grouping changes with the height in every case; held to the rounding of
    those sums.

Shapes that are not registered at build time (csrc/shapes.hpp) are staged with the run-time build of their
shape plugin switched off (a hipcc run of minutes; tests/test_gpu_jit.py covers the plugins): for them both
settings of AMPC_STATIC run the run-time-shape kernels."""
import numpy as np
import pytest

from helpers import make_system, rel_err
from oracle import mlp as omlp
from oracle.costs import QuadCostOracle
from oracle.mppi import MPPIOracle

pytestmark = pytest.mark.gpu

# (nx, nu, hidden, activation, tile heights that must run: every listed height fits the 160 KB of LDS)
CASES = [
    (2, 1, [64, 64], "relu", (16, 32, 64)),              # W = 4, registered shape
    (17, 6, [128, 128], "relu", (16, 32, 64)),           # W = 8, NT = 1
    (17, 6, [256, 256], "relu", (16, 32, 64)),           # the headline instantiation, 4x4x4 output tail
    (3, 2, [32], "relu", (16, 32, 64)),                  # one hidden layer
    (5, 3, [64, 48, 64], "sigmoid", (16, 32, 64)),       # a third hidden layer (beyond the resident biases), padded width
    (7, 2, [16, 32, 64, 16], "selu", (16, 32, 64)),      # four hidden layers
    (30, 2, [64, 64], "tanh", (16, 32, 64)),             # two output tiles
]
REGISTERED = {(17, 6, (256, 256)), (2, 1, (64, 64)), (4, 1, (64, 64)), (17, 6, (128, 128))}
N, H = np.array([37, 130]), np.array([9, 6])          # two problems, ragged tiles
SIGMA, LMDA = np.array([0.3, 0.6]), np.array([0.7, 1.3])


def costs_bitwise(nx, nu, hidden, rows):
    """Are a sample's cost terms grouped on `rows`-row tiles as on 16-row tiles?  (module docstring)"""
    hpad = (max(hidden) + 63) // 64 * 64
    waves = 8 if hpad % 128 == 0 else 4                 # (csrc/shapes.hpp: 64 -> 4, 128 -> 8, 192 -> 4, 256 -> 8)
    return max(nx, nu) <= 64 * waves // rows


def _big_bias_params(nx, nu, hidden, act, seed):
    """torch-default weights, each hidden layer scaled until its weighted sums (on a batch of O(0.3) inputs)
    have rms 1e-3, under biases N(0, 1): 1e3 x the sums, activations not saturated.  The output layer is
    scaled so that a step moves the state by O(0.1): the states stay O(1) over the horizon."""
    p = omlp.random_params(nx, nu, hidden, act, seed=seed)
    rng = np.random.default_rng(seed + 100)
    a = rng.normal(size=(256, nx + nu)) * 0.3
    for l in range(len(hidden)):
        z = a @ p["weights"][l].T
        p["weights"][l] = p["weights"][l] * (1e-3 / np.sqrt(np.mean(z * z)))
        p["biases"][l] = rng.normal(size=hidden[l])
        a = omlp.act_fn(act, a @ p["weights"][l].T + p["biases"][l])
    y = a @ p["weights"][-1].T
    p["weights"][-1] = p["weights"][-1] / np.sqrt(np.mean(y * y))
    p["biases"][-1] = rng.normal(size=nx) * 0.1
    return p


def _handle(p, nx, nu, act, precision, jit):
    from autompc_amd import _lib
    h = _lib.Handle(0, precision, jit=jit)
    h.set_mlp(nx, nu, p["weights"], p["biases"], act, p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"])
    return h


def _solve(h, rows, x0, act_seq, eps):
    """One solve on `rows`-row tiles; None if that height does not fit LDS for the model."""
    from autompc_amd import _lib
    plan = _lib.MppiPlan(h, N, H, SIGMA, LMDA)
    try:
        plan.set_geometry(rows, 0)
    except _lib.AmpcError:
        plan.close()
        return None
    plan.upload(x0=x0, act_seq=act_seq, eps=eps)
    plan.solve()
    a, _, c, _ = plan.download(costs=True)
    kind, spw = plan.kernel_kind(), plan.info()["samples_per_wg"]
    plan.close()
    return a, c, kind, spw


@pytest.mark.parametrize("nx,nu,hidden,act,must_run", CASES)
def test_bias_dominated_networks(nx, nu, hidden, act, must_run, monkeypatch):
    from autompc_amd import _lib
    monkeypatch.delenv("AMPC_MT", raising=False)
    monkeypatch.setenv("AMPC_STATIC", "1")
    registered = (nx, nu, tuple(hidden)) in REGISTERED
    p = _big_bias_params(nx, nu, hidden, act, seed=nx + len(hidden))
    rng = np.random.default_rng(17 + nx)
    Q, R, F = np.diag(rng.uniform(0.5, 2, nx)), np.diag(rng.uniform(0.01, 0.1, nu)), np.diag(rng.uniform(0.5, 3, nx))
    goal = rng.normal(size=nx) * 0.1
    lo, hi = -rng.uniform(0.3, 1.0, nu), rng.uniform(0.5, 1.0, nu)
    x0 = rng.normal(size=(2, nx)) * 0.2
    act_seq = rng.uniform(-0.3, 0.3, size=int(np.sum(H * nu)))
    eps = np.concatenate([rng.normal(size=N[b] * H[b] * nu) * np.sqrt(SIGMA[b]) for b in range(2)])
    S, C = rng.normal(size=(45, nx)) * 0.3, rng.normal(size=(45, nu)) * 0.3

    # ---- the reference, once: pred_batch / pred_diff_batch and the two problems' solves --------------------
    ref_o, ref_jx, ref_ju = omlp.pred_diff_batch(p, S, C)
    # (what the test is about: without its biases the network predicts something else entirely)
    q = dict(p, biases=[np.zeros_like(b) for b in p["biases"][:-1]] + [p["biases"][-1]])
    assert rel_err(omlp.pred_batch(q, S, C) - S, ref_o - S) > 0.1
    model = omlp.MLPOracle(make_system(nx, nu), p)
    ref_c, ref_a = [], []
    off_a = off_e = 0
    for b in range(2):
        n, hh = int(N[b]), int(H[b])
        orc = MPPIOracle(model, QuadCostOracle(Q, R, F, goal), np.stack([lo, hi], axis=1), horizon=hh, num_path=n,
                         sigma=float(SIGMA[b]), lmda=float(LMDA[b]))
        orc.act_sequence = act_seq[off_a:off_a + hh * nu].reshape(hh, nu).copy()
        costs, e = orc.do_rollouts(x0[b], eps[off_e:off_e + n * hh * nu].reshape(n, hh, nu))
        orc.update(costs, e)
        ref_c.append(costs); ref_a.append(orc.act_sequence.reshape(-1))
        off_a += hh * nu; off_e += n * hh * nu

    def check_against_oracle(a, c, tol_c, tol_a):
        oc = oa = 0
        for b in range(2):
            n, hh = int(N[b]), int(H[b])
            ec, ea = rel_err(c[oc:oc + n], ref_c[b]), rel_err(a[oa:oa + hh * nu], ref_a[b])
            print("  problem %d: cost rel err %.2e  sequence rel err %.2e" % (b, ec, ea))
            assert ec < tol_c and ea < tol_a
            oc += n; oa += hh * nu

    # ---- f64: prediction, Jacobians, solve ----------------------------------------------------------------
    h = _handle(p, nx, nu, act, "f64", jit=False)
    h.set_quad_costs(Q, R, F, goal)
    h.set_ctrl_bounds(lo, hi)
    o = h.pred_batch(S, C)
    o2, jx, ju = h.pred_diff_batch(S, C)
    eye = np.eye(nx)[None]
    errs = rel_err(o, ref_o), rel_err(o2, ref_o), rel_err(ju, ref_ju)
    # jx - I: off the diagonal it is the network's Jacobian itself; a diagonal entry is 1 + J_ii rounded to f64 on
    # either side, 1.1e-16 each, whatever the size of J_ii
    dx, sx = np.abs(jx - ref_jx), float(np.max(np.abs(ref_jx - eye)))
    on, off = float(np.max(dx * eye)), float(np.max(dx * (1 - eye)))
    print("pred_batch %.2e  pred_diff_batch %.2e  ju %.2e (max |ju| %.1e)  jx - I: off-diagonal %.2e diagonal %.2e, max %.1e"
          % (errs + (np.max(np.abs(ref_ju)), off, on, sx)))
    assert max(errs) < 1e-10 and off < 1e-10 * sx and on < 1e-10 * sx + 2.3e-16
    a16, c16, kind, spw = _solve(h, 16, x0, act_seq, eps)
    assert spw == 16 and (kind == 1 if registered else kind in (0, 2))     # (2: a plugin cached by an earlier run)
    check_against_oracle(a16, c16, 1e-10, 1e-9)

    # ---- tile heights (module docstring) -----------------------------------------------------------------------
    for mt in ("1", "2", "4"):
        monkeypatch.setenv("AMPC_MT", mt)
        hm = _handle(p, nx, nu, act, "f64", jit=False)
        np.testing.assert_array_equal(hm.pred_batch(S, C), o)
        hm.close()
    monkeypatch.delenv("AMPC_MT")
    for rows in (32, 64):
        res = _solve(h, rows, x0, act_seq, eps)
        if res is None:
            assert rows not in must_run, "%d-row tiles no longer fit" % rows
            continue
        a, c, _, spw = res
        assert spw == rows
        bitwise = costs_bitwise(nx, nu, hidden, rows)
        print("  %d-row tiles vs 16-row tiles: costs %.2e (%s)  sequence %.2e"
              % (rows, rel_err(c, c16), "same grouping" if bitwise else "regrouped", rel_err(a, a16)))
        if bitwise:
            np.testing.assert_array_equal(c, c16)
        else:
            # <= 9 * (nx + nu) + nx <= 300 non-negative terms (diagonal Q, R, F): two groupings differ by at
            # most ~300 x 1.1e-16 of the sum
            assert rel_err(c, c16) < 1e-13
        # <= 130 weighted noise values per element, one partial sum per tile: ~130 x 1.1e-16 x sum |w e| / |sum w e|,
        # below 1e-12 for any sum that does not cancel to less than 1 % of its terms
        assert rel_err(a, a16) < 1e-12
    # ---- shape-specialised vs run-time-shape kernels: the same bits -----------------------------------------
    monkeypatch.setenv("AMPC_STATIC", "0")
    a, c, kind, _ = _solve(h, 16, x0, act_seq, eps)
    assert kind == 0
    np.testing.assert_array_equal(c, c16)
    np.testing.assert_array_equal(a, a16)
    monkeypatch.setenv("AMPC_STATIC", "1")
    h.close()

    # ---- f32 follows f64 ------------------------------------------------------------------------------------
    h32 = _handle(p, nx, nu, act, "f32", jit=False)
    h32.set_quad_costs(Q, R, F, goal)
    h32.set_ctrl_bounds(lo, hi)
    e32 = rel_err(h32.pred_batch(S, C), o)
    a32, c32, _, _ = _solve(h32, 16, x0, act_seq, eps)
    print("f32 vs f64: pred_batch %.2e  costs %.2e  sequence %.2e" % (e32, rel_err(c32, c16), rel_err(a32, a16)))
    assert e32 < 1e-4 and rel_err(c32, c16) < 1e-4 and rel_err(a32, a16) < 1e-4
    h32.close()
