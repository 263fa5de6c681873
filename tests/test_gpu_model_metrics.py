"""k-step model accuracy on the MI355X (ampc_kstep_errors, csrc/kstep_kernels.hpp): the reference's
get_model_rmse / get_model_rmsmens of seeded MLPs and of reference-trained ARX / Koopman models
(tests/golden/kstep_*.npz), the device sums against the host composition over the same handle's pred_batch,
determinism, batching, input order and f32.  Needs MI355X."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden
from helpers import golden_params, make_system, weight_checksum

pytestmark = pytest.mark.gpu

MLP_TAGS = sorted(os.path.basename(p)[len("kstep_mlp_"):-4] for p in glob.glob(os.path.join(GOLDEN, "kstep_mlp_*.npz")))


def _trajs(system, g):
    from autompc_amd import Trajectory
    out, o = [], 0
    for L in g["lens"]:
        L = int(L)
        out.append(Trajectory(system, L, g["obs"][o:o + L].copy(), g["ctrls"][o:o + L].copy()))
        o += L
    return out


def _mlp(system, p, hidden, act, precision="f64"):
    from autompc_amd import MLP
    m = MLP(system, n_hidden_layers=len(hidden), nonlintype=str(act), precision=precision,
            **{"hidden_size_%d" % (i + 1): int(h) for i, h in enumerate(hidden)})
    m.jit_kernels = False
    m.weights, m.biases = [w.copy() for w in p["weights"]], [b.copy() for b in p["biases"]]
    m.xu_means, m.xu_std, m.dy_means, m.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
    return m


def _fixture_model(tag, precision="f64", seed=None):
    g = golden("kstep_mlp_" + tag)
    nx, nu = int(g["nx"]), int(g["nu"])
    system = make_system(nx, nu)
    p = golden_params(nx, nu, g["hidden"], str(g["activation"]), int(g["seed"]) if seed is None else seed)
    if seed is None:
        np.testing.assert_allclose(weight_checksum(p), g["checksum"], rtol=0, atol=1e-12)
    return _mlp(system, p, g["hidden"], g["activation"], precision), _trajs(system, g), g


@pytest.mark.parametrize("tag", MLP_TAGS)
def test_mlp_fixtures_every_horizon_both_metrics(tag):
    from autompc_amd.evaluation import model_errors
    from autompc_amd.evaluation.model_metrics import device_shape_key
    model, trajs, g = _fixture_model(tag)
    assert device_shape_key(model) is not None
    hs = [int(h) for h in g["horizons"]]
    rmse = model_errors([model], trajs, hs, "rmse")[0]
    rmsmens = model_errors([model], trajs, hs, "rmsmens")[0]
    dev = max(np.max(np.abs(rmse / g["rmse"] - 1)), np.max(np.abs(rmsmens / g["rmsmens"] - 1)))
    print("kstep %s: largest relative deviation from the reference %.2e" % (tag, dev))
    np.testing.assert_allclose(rmse, g["rmse"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(rmsmens, g["rmsmens"], rtol=1e-9, atol=0)


@pytest.mark.parametrize("tag", ["hc_relu2", "c4_sigmoid3", "w64_sigmoid2"])
def test_device_sums_equal_host_composition_over_pred_batch(tag):
    from autompc_amd.evaluation.model_metrics import host_rmse, host_rmsmens, model_errors
    model, trajs, g = _fixture_model(tag)
    hs = [1, 2, 5, 20]
    dev = model_errors([model], trajs, hs, "rmse")[0]
    host = np.array([host_rmse(model, trajs, h) for h in hs])        # the reference loop over this handle
    np.testing.assert_allclose(dev, host, rtol=1e-12, atol=0)
    dev_m = model_errors([model], trajs, hs, "rmsmens")[0]
    host_m = np.array([host_rmsmens(model, trajs, h) for h in hs])
    np.testing.assert_allclose(dev_m, host_m, rtol=1e-12, atol=0)
    print("kstep %s vs pred_batch: rmse bitwise equal %s (max rel %.1e), rmsmens bitwise equal %s (max rel %.1e)"
          % (tag, np.array_equal(dev, host), np.max(np.abs(dev / host - 1)), np.array_equal(dev_m, host_m),
             np.max(np.abs(dev_m / host_m - 1))))


def test_repeatable_batched_and_in_input_order():
    from autompc_amd.evaluation.model_metrics import kstep_sums, model_errors
    g = golden("kstep_mlp_hc_relu2")
    nx, nu = int(g["nx"]), int(g["nu"])
    system = make_system(nx, nu)
    trajs = _trajs(system, g)
    models = [_mlp(system, golden_params(nx, nu, g["hidden"], "relu", 100 + k), g["hidden"], "relu")
              for k in range(8)]
    S1, D1 = kstep_sums(models, trajs, 12, delta=True)
    S2, D2 = kstep_sums(models, trajs, 12, delta=True)
    assert np.array_equal(S1, S2) and np.array_equal(D1, D2)                 # run to run
    for k, m in enumerate(models):
        S, D = kstep_sums([m], trajs, 12, delta=True)
        assert np.array_equal(S[0], S1[k]) and np.array_equal(D[0], D1[k])  # one call of eight = eight calls
    assert len({S1[k, 3] for k in range(8)}) == 8
    # a mixed-shape list comes back in input order
    other, _, _ = _fixture_model("hc_tanh1")
    mixed = [models[0], other, models[1], other]
    out = model_errors(mixed, trajs, [1, 4, 12], "rmse")
    for k, m in enumerate(mixed):
        np.testing.assert_array_equal(out[k], model_errors([m], trajs, [1, 4, 12], "rmse")[0])


def _linear(tag):
    from autompc_amd import ARX, Koopman
    g = golden("kstep_lin_" + tag)
    system = make_system(int(g["nx"]), int(g["nu"]))
    if tag.startswith("arx"):
        m = ARX(system, history=int(tag[3]))
    else:
        m = Koopman(system, method="lstsq", poly_basis=True, poly_degree=2)
    assert m.state_dim == int(g["state_dim"])
    m.A, m.B = g["A"].copy(), g["B"].copy()
    return m, _trajs(system, g), g


@pytest.mark.parametrize("tag", ["arx2", "arx4", "koop_poly", "arx4_wide"])
def test_linear_models(tag):
    from autompc_amd.evaluation import model_errors
    from autompc_amd.evaluation.model_metrics import device_shape_key
    m, trajs, g = _linear(tag)
    assert (device_shape_key(m) is None) == (tag == "arx4_wide")           # the wide ARX takes the host fallback
    out = model_errors([m], trajs, [int(h) for h in g["horizons"]], "rmse")[0]
    print("kstep %s: largest relative deviation from the reference %.2e" % (tag, np.max(np.abs(out / g["rmse"] - 1))))
    np.testing.assert_allclose(out, g["rmse"], rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        model_errors([m], trajs, [1], "rmsmens")                            # the state is not the observation


def test_f32_handle_agrees_with_f64():
    """An f32 model carries about 1e-7 relative error per step in its state (f32 weights and state, exact
    f32 MFMA); over 20 steps of a net whose per-step Jacobian is near the identity the error grows roughly
    linearly, and the RMSE compares states with a spread of ~1, so 1e-4 relative bounds it with margin while
    still catching any indexing or precision-mixing slip (those give O(1) differences)."""
    from autompc_amd.evaluation import model_errors
    m64, trajs, g = _fixture_model("hc_relu2")
    m32, _, _ = _fixture_model("hc_relu2", precision="f32")
    hs = [int(h) for h in g["horizons"]]
    a = model_errors([m64], trajs, hs, "rmse")[0]
    b = model_errors([m32], trajs, hs, "rmse")[0]
    print("kstep f32 vs f64: max rel %.2e" % np.max(np.abs(b / a - 1)))
    np.testing.assert_allclose(b, a, rtol=1e-4)
    assert not np.array_equal(a, b)
