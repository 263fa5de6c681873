"""The host side of the wide-linear k-step path (ampc_kstep_errors_linear, evaluation/model_metrics.py): the ABI,
the state rules against traj_to_states, the grouping, and the ``linear_kstep`` option.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from autompc_amd import ARX, Koopman
from autompc_amd.evaluation import model_metrics as MM
from kstep_wide_cases import RULES, WIDE, ObsLinear, RowsARX, ragged_trajs, system, wide_model


def test_abi_exports_and_binds_the_entry():
    from autompc_amd import _lib
    from autompc_amd.csrc.build import build
    lib = ctypes.CDLL(build(verbose=False))
    assert hasattr(lib, "ampc_kstep_errors_linear")
    assert "ampc_kstep_errors_linear" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ampc_kstep_errors_linear"][1]) == 17
    assert _lib.load().ampc_version() >= 111
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "autompc_hip.h")).read()
    assert "ampc_kstep_errors_linear(" in header


@pytest.mark.parametrize("shape", [(17, 6), (3, 1), (20, 1)])
def test_arx_rule_is_traj_to_states_bit_for_bit(shape):
    """Histories 1..10 on ragged trajectories, one-row ones included, and on every prefix the reference's loop
    passes (a feature looks backwards only, so a prefix's states are the full trajectory's rows)."""
    s = system(*shape)
    trajs = ragged_trajs(s, [31, 1, 19, 2, 3, 12, 1, 45], 5)
    for k in range(1, 11):
        m = ARX(s, history=k)
        rule = MM.linear_state_rule(m)
        assert rule == {"rule": 1, "history": k}
        for t in trajs:
            want = m.traj_to_states(t)
            got = MM.rule_states(rule, t.obs, t.ctrls)
            assert got.shape == (len(t), m.state_dim) and np.array_equal(got, want)
            for cut in (1, 5, 20):
                if len(t) > cut:
                    assert np.array_equal(m.traj_to_states(t[:-cut]), got[:-cut])


def test_koopman_rule_agrees_with_apply_basis():
    s = system(17, 6)
    trajs = ragged_trajs(s, [25, 1, 9], 6)
    for kw in (dict(), dict(poly_basis=True, poly_degree=3), dict(trig_basis=True, poly_degree=2),
               dict(poly_basis=True, poly_degree=4, trig_basis=True, trig_freq=3, strict_reference=False)):
        m = Koopman(s, **kw)
        rule = MM.linear_state_rule(m)
        assert rule["rule"] == 2 and len(rule["kinds"]) * 17 == m.state_dim
        assert rule["kinds"].dtype == np.int32 and rule["params"].dtype == np.float64
        for t in trajs:
            np.testing.assert_array_equal(MM.rule_states(rule, t.obs, t.ctrls), m.traj_to_states(t))
    assert MM.linear_state_rule(Koopman(s, product_terms=True)) == {"rule": 0}      # not expressible: rows
    assert MM.linear_state_rule(RowsARX(s, history=4)) == {"rule": 0}               # its own traj_to_states: rows
    assert MM.linear_state_rule(ObsLinear(system(70, 2))) == {"rule": 0}
    with pytest.raises(ValueError):
        MM.rule_states({"rule": 0}, trajs[0].obs, trajs[0].ctrls)


@pytest.mark.parametrize("tag", sorted(WIDE))
def test_golden_models_take_their_rule_and_the_wide_group(tag):
    m, trajs, g = wide_model(tag)
    assert MM.linear_state_rule(m)["rule"] == RULES[tag]
    assert MM.device_shape_key(m) is None                      # ampc_kstep_errors still refuses them
    assert MM.wide_linear_key(m) == ("wide-linear", "f64", 0, int(g["nu"]))


def test_wide_group_membership():
    s = system(17, 6)
    narrow = ARX(s, history=2)
    narrow.A, narrow.B = np.zeros((41, 41)), np.zeros((41, 6))
    assert MM.wide_linear_key(narrow) is None and MM.device_shape_key(narrow) is not None
    assert MM.wide_linear_key(ARX(s, history=4)) is None       # untrained

    class Foreign(ARX):
        def pred_batch(self, states, ctrls):
            return states

    f = Foreign(s, history=4)
    f.A, f.B = np.zeros((87, 87)), np.zeros((87, 6))
    assert MM.wide_linear_key(f) is None
    big = ObsLinear(system(300, 2))
    big.A, big.B = np.zeros((300, 300)), np.zeros((300, 2))
    assert MM.wide_linear_key(big) is None                     # beyond ampc_set_linear: host fallback, counted
    # the delta sums' error blocks of a very wide observation do not fit LDS beside the operand buffers
    wide = ObsLinear(system(240, 2))
    wide.A, wide.B = np.zeros((240, 240)), np.zeros((240, 2))
    assert MM.wide_linear_key(wide) is not None and MM.wide_linear_key(wide, delta=True) is None
    a, b = wide_model("arx4_hc")[0], wide_model("arx10_hc", precision="f32")[0]
    assert MM.wide_linear_key(a) != MM.wide_linear_key(b)      # precisions do not share a call
    assert MM.wide_linear_key(a) == MM.wide_linear_key(wide_model("koop_polytrig")[0])   # state dims may differ


def test_linear_kstep_option_is_checked_and_the_default_stays_on_the_old_entries(monkeypatch):
    from autompc_amd.evaluation import HoldoutModelEvaluator, get_model_rmse, get_model_rmsmens, model_errors
    s = system(3, 1)
    trajs = ragged_trajs(s, [12, 9, 15, 11], 7)
    for bad in ("gpu", None, "Device"):
        with pytest.raises(ValueError):
            model_errors([], trajs, [1], "rmse", linear_kstep=bad)
        with pytest.raises(ValueError):
            HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(0), linear_kstep=bad)
    ev = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(0))
    assert ev.linear_kstep == "host" and ev.linear_fit == "host"
    assert HoldoutModelEvaluator(s, trajs, "rmsmens", np.random.default_rng(0),
                                 linear_kstep="device").linear_kstep == "device"

    def boom(*a, **k):
        raise AssertionError("the default path must not reach the wide-linear entry")

    monkeypatch.setattr(MM, "kstep_sums_linear", boom)
    monkeypatch.setattr(MM, "wide_linear_key", boom)

    class NumpyLinear:
        """A foreign model: the host fallback without a GPU."""
        def __init__(self, system, A, B):
            self.system, self.A, self.B = system, A, B

        def pred_batch(self, states, ctrls):
            return states @ self.A.T + ctrls @ self.B.T

    rng = np.random.default_rng(1)
    m = NumpyLinear(s, np.eye(3) + 0.05 * rng.normal(size=(3, 3)), 0.1 * rng.normal(size=(3, 1)))
    rep = MM.KstepReport()
    out = model_errors([m, m], trajs, [1, 3], "rmse", report=rep)
    assert rep.host_fallbacks == 2 and rep.wide_models == 0 and rep.device_models == 0 and MM.last_report is rep
    assert out[0, 1] == MM.host_rmse(m, trajs, 3) == get_model_rmse(m, trajs, 3)
    assert get_model_rmsmens(m, trajs, 2) == MM.host_rmsmens(m, trajs, 2)
