"""The host side of the SINDy k-step path (ampc_kstep_errors_sindy, evaluation/model_metrics.py): the ABI, the
grouping key, the ``sindy_kstep`` option, and the goldens of tests/golden/gen_golden_kstep_sindy.py against the
oracle's numpy SINDy over the host loop.  No GPU.

Tolerance of the golden check: 1e-9 relative, the project's k-step bound.  The numpy composition reproduces the
reference's value to 2.2e-16 .. 8.9e-16 (gen_golden_kstep_sindy.py prints it), so all of it is rounding allowance.
"""
import ctypes
import os

import numpy as np
import pytest

from autompc_amd import SINDy
from autompc_amd.evaluation import model_metrics as MM
from kstep_sindy_cases import CASES, hyper_of, sindy_model, system
from oracle.sindy import SINDyOracle


def test_abi_exports_and_binds_the_entry():
    from autompc_amd import _lib
    from autompc_amd.csrc.build import build
    lib = ctypes.CDLL(build(verbose=False))
    assert hasattr(lib, "ampc_kstep_errors_sindy")
    assert len(_lib.SIGNATURES["ampc_kstep_errors_sindy"][1]) == 11
    assert _lib.load().ampc_version() >= 112
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "autompc_hip.h")).read()
    assert "ampc_kstep_errors_sindy(" in header


@pytest.mark.parametrize("tag", sorted(CASES))
def test_golden_models_take_the_sindy_group_and_their_program_form(tag):
    m, trajs, g = sindy_model(tag)
    nx, nu = int(g["nx"]), int(g["nu"])
    assert MM.device_shape_key(m) is None                      # ampc_kstep_errors still refuses them
    assert MM.wide_linear_key(m) is None
    for delta in (False, True):
        assert MM.sindy_kstep_key(m, nx, delta) == ("sindy", "f64", 0, nx, nu)
    n_feat, n_trig, n_pow, n_mon, n_pool, n_tab = MM.sindy_program_sizes(m)
    table, staged = CASES[tag]
    assert n_feat == g["Xi"].shape[1] and (n_tab > 0) == table
    assert n_tab == (2 * n_trig + n_pow + n_mon + 1 if table else 0) and n_tab <= 160
    # the staged program is what the LDS bytes carry beyond the columns and the error block
    cols = (2 * nx + nu + n_tab) * 64 * 8 + 8 * 65 * 8
    assert (MM._sindy_lds_bytes(m, nx, nu, False) > cols) == staged
    assert MM._sindy_lds_bytes(m, nx, nu, True) - MM._sindy_lds_bytes(m, nx, nu, False) == 8 * 65 * 8


def test_sindy_group_membership():
    a, _, _ = sindy_model("cross3")
    b, _, _ = sindy_model("poly3_trig2_cont")
    c, _, _ = sindy_model("cross5")
    assert MM.sindy_kstep_key(a) == MM.sindy_kstep_key(b) == MM.sindy_kstep_key(c) == ("sindy", "f64", 0, 3, 2)
    assert MM.sindy_kstep_key(sindy_model("cross3", precision="f32")[0]) == ("sindy", "f32", 0, 3, 2)
    assert MM.sindy_kstep_key(sindy_model("c1_trig")[0]) == ("sindy", "f64", 0, 4, 1)
    assert MM.sindy_kstep_key(a, obs_dim=4) is None            # data of another system

    class Foreign(SINDy):
        def pred_batch(self, states, ctrls):
            return states

    assert MM.sindy_kstep_key(Foreign(system(3, 2))) is None
    assert MM.sindy_kstep_key(SINDyOracle(system(3, 2), np.zeros((3, 5)))) is None
    from kstep_wide_cases import wide_model
    assert MM.sindy_kstep_key(wide_model("arx4_hc")[0]) is None
    assert MM.sindy_kstep_key(SINDy(system(65, 2))) is None    # beyond ampc_set_sindy


def test_lds_bytes_follow_the_kernel_layout(monkeypatch):
    """The widest program SINDy's own libraries give: 64 / 15 with one trig frequency has 79 sin / cos arguments, a
    table of 159 entries, 2 * 64 + 15 + 159 = 302 f64 columns of 64 rows and a program too large to stage.  It fits
    the 160 KB (only a hand-made 64 / 16 program with exactly 160 table entries and the delta block does not); one
    more variable makes the table 161 entries, and the model is evaluated directly with no table columns at all."""
    big = SINDy(system(64, 15), trig_basis=True, trig_freq=1)
    assert MM.sindy_program_sizes(big) == (237, 79, 0, 0, 0, 159)
    assert MM._sindy_lds_bytes(big, 64, 15, False) == 302 * 64 * 8 + 8 * 65 * 8
    assert MM._sindy_lds_bytes(big, 64, 15, True) == 302 * 64 * 8 + 2 * 8 * 65 * 8 <= 160 * 1024
    assert MM.sindy_kstep_key(big, delta=True) == ("sindy", "f64", 0, 64, 15)
    direct = SINDy(system(64, 16), trig_basis=True, trig_freq=1)
    assert MM.sindy_program_sizes(direct) == (240, 0, 0, 0, 0, 0)
    assert MM._sindy_lds_bytes(direct, 64, 16, False) == 144 * 64 * 8 + 8 * 65 * 8
    # a staged program: c1_trig's 55 x 4 coefficients, 5 frequencies, 2 x 55 + 5 table indices, f64
    small, _, _ = sindy_model("c1_trig")
    assert MM.sindy_program_sizes(small) == (55, 5, 0, 0, 0, 11)
    elems = 55 * 4 + 5 + ((2 * 55 + 5) * 4 + 7) // 8 + 2        # sindy_prog_elems
    assert MM._sindy_lds_bytes(small, 4, 1, False) == (2 * 4 + 1 + 11) * 64 * 8 + 8 * 65 * 8 + (elems + 2) * 8
    # a model that does not fit is not keyed: it takes the host loop and is counted there
    monkeypatch.setattr(MM, "_LDS_BYTES", 302 * 64 * 8 + 8 * 65 * 8)
    assert MM.sindy_kstep_key(big) is not None and MM.sindy_kstep_key(big, delta=True) is None


class _Counting(SINDyOracle):
    calls = 0

    def pred_batch(self, states, ctrls):
        type(self).calls += 1
        return super().pred_batch(states, ctrls)


def test_sindy_kstep_option_is_checked_and_the_default_stays_on_the_host_loop(monkeypatch):
    from autompc_amd.evaluation import HoldoutModelEvaluator, get_model_rmse, get_model_rmsmens, model_errors
    _, trajs, g = sindy_model("cross3")
    s = trajs[0].system
    for bad in ("gpu", None, "Device"):
        with pytest.raises(ValueError, match="sindy_kstep"):
            model_errors([], trajs, [1], "rmse", sindy_kstep=bad)
        with pytest.raises(ValueError, match="sindy_kstep"):
            HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(0), sindy_kstep=bad)
        with pytest.raises(ValueError, match="sindy_kstep"):
            get_model_rmse(None, trajs, 1, sindy_kstep=bad)
    ev = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(0))
    assert ev.sindy_kstep == "host" and ev.linear_kstep == "host"
    assert HoldoutModelEvaluator(s, trajs, "rmsmens", np.random.default_rng(0),
                                 sindy_kstep="device").sindy_kstep == "device"

    def boom(*a, **k):
        raise AssertionError("the default path must not reach the SINDy entry")

    monkeypatch.setattr(MM, "kstep_sums_sindy", boom)
    monkeypatch.setattr(MM, "sindy_kstep_key", boom)
    h = hyper_of(g)
    m = _Counting(s, g["Xi"], trig_freq=0, poly_degree=h["poly_degree"], poly_cross_terms=True)
    r0, r1 = MM.KstepReport(), MM.KstepReport()
    a = model_errors([m, m], trajs, [1, 3, 20], "rmse", report=r0)
    n0 = _Counting.calls
    b = model_errors([m, m], trajs, [1, 3, 20], "rmse", report=r1, sindy_kstep="host")
    assert _Counting.calls == 2 * n0 and np.array_equal(a, b) and MM.last_report is r1
    assert vars(r0) == vars(r1) and r0.host_fallbacks == 2 and r0.sindy_models == 0 and r0.sindy_calls == 0
    assert "sindy_models=0, sindy_calls=0" in repr(r0)
    assert a[0, 1] == MM.host_rmse(m, trajs, 3) == get_model_rmse(m, trajs, 3) == get_model_rmse(m, trajs, 3,
                                                                                                  sindy_kstep="host")
    assert get_model_rmsmens(m, trajs, 2, sindy_kstep="host") == MM.host_rmsmens(m, trajs, 2)
    monkeypatch.undo()
    # a foreign model stays on the host loop with the option on, and is counted
    r2 = MM.KstepReport()
    c = model_errors([m], trajs, [1, 3, 20], "rmse", report=r2, sindy_kstep="device")
    assert np.array_equal(c[0], a[0]) and r2.host_fallbacks == 1 and r2.sindy_models == 0


@pytest.mark.parametrize("tag", sorted(CASES))
def test_goldens_against_the_oracle_over_the_host_loop(tag):
    _, trajs, g = sindy_model(tag)
    m = SINDyOracle(trajs[0].system, g["Xi"], trig_freq=int(g["trig_freq"]),
                    trig_interaction=bool(g["trig_interaction"]), poly_degree=int(g["poly_degree"]),
                    time_mode=str(g["time_mode"]), poly_cross_terms=bool(g["poly_cross_terms"]))
    assert [len(t) for t in trajs] == [31, 19, 38, 20, 29, 45, 3, 1]
    assert MM.row_counts(trajs, 1)[0] == 178                   # three 64-row tiles, the last partial
    hs = [int(h) for h in g["horizons"]]
    rmse = np.array([MM.host_rmse(m, trajs, h) for h in hs])
    rmsmens = np.array([MM.host_rmsmens(m, trajs, h) for h in hs])
    print("kstep sindy %s: oracle over the host loop vs the reference: rmse %.1e, rmsmens %.1e"
          % (tag, np.max(np.abs(rmse / g["rmse"] - 1)), np.max(np.abs(rmsmens / g["rmsmens"] - 1))))
    np.testing.assert_allclose(rmse, g["rmse"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(rmsmens, g["rmsmens"], rtol=1e-9, atol=0)
