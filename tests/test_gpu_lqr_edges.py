"""The LQR gain kernel and closed loop at their tile edges and limits, with diagonal, non-symmetric and pivoting
costs (tests/lqr_edge_cases.py), against the reference's recursion in long double (tests/golden/lqr_edges.npz,
gen_golden_lqr_edges.py).  Tolerance, per case: max(100 x host_err, 1e-13) of max|K|, host_err being what the f64 host
form loses against the same long-double gain (the project's rule).  Needs MI355X."""
import numpy as np
import pytest

from autompc_amd import _lib
import lqr_edge_cases as E

pytestmark = pytest.mark.gpu


def _checked_case(name):
    """The case's inputs, after their checksum: a drifted random stream fails here, not as a tolerance."""
    arrays = E.make_case(name)
    np.testing.assert_array_equal(E.checksum(arrays), E.fixture()["checksum_" + name])
    return arrays


def _handle(A, B):
    h = _lib.Handle(0, "f64")
    h.set_linear(A, B)
    return h


def _gains(names):
    """(K list, status) of the cases `names` (one (no, nu)) in one plan."""
    cases = [_checked_case(nm) for nm in names]
    c0 = E.CASES[names[0]]
    handles = [_handle(A, B) for A, B, _, _, _ in cases]
    plan = _lib.LqrPlan(handles, c0["no"], c0["nu"])
    try:
        return plan.gains([E.CASES[nm]["horizon"] for nm in names], np.array([c[2] for c in cases]),
                          np.array([c[3] for c in cases]), np.array([c[4] for c in cases]))
    finally:
        plan.close()
        for h in handles:
            h.close()


_alone = {}


def _gain_alone(name):
    if name not in _alone:
        K, status = _gains([name])
        _alone[name] = (K[0], int(status[0]))
    return _alone[name]


@pytest.mark.parametrize("name", list(E.CASES))
def test_gain_against_long_double(name):
    K, status = _gain_alone(name)
    assert status == 0
    fx = E.fixture()
    ref, host_err = fx["K_" + name], float(fx["host_err_" + name])
    err, tol = E.rel_err(K, ref), E.tolerance(host_err)
    print("%-24s host_err %.1e  device %.1e  tolerance %.1e" % (name, host_err, err, tol))
    assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("group", [g for g in E.plan_groups().values() if len(g) > 1], ids=lambda g: g[0])
def test_gains_independent_of_the_plan(group):
    K, status = _gains(group)
    assert np.all(status == 0)
    for i, name in enumerate(group):
        assert np.array_equal(K[i], _gain_alone(name)[0]), name
    Kr, _ = _gains(group[::-1])
    for i, name in enumerate(group[::-1]):
        assert np.array_equal(Kr[i], _gain_alone(name)[0]), name


def test_singular_gain_at_16_controls():
    """R of rank 15 (a zero on its diagonal) and F = Q = 0, so B'PB = 0 and R + B'PB is R: status 1 and a NaN gain,
    where the reference's inversion raises; the healthy problem beside it in the plan keeps its bits."""
    name = "n256_u16_o17_diag"
    A, B, Q, R, F = _checked_case(name)
    Rs = np.diag(np.arange(1.0, 17.0))
    Rs[7, 7] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        E.riccati(A, B, 0 * Q, Rs, 0 * F, 2, dtype=np.float64)
    h = _handle(A, B)
    plan = _lib.LqrPlan([h, h], 17, 16)
    K, status = plan.gains([2, E.CASES[name]["horizon"]], np.array([0 * Q, Q]), np.array([Rs, R]),
                           np.array([0 * F, F]))
    plan.close()
    h.close()
    assert status[0] == 1 and np.all(np.isnan(K[0]))
    assert status[1] == 0 and np.array_equal(K[1], _gain_alone(name)[0])


# ---- closed loop: lqr_ctrl_kernel / lqr_record_kernel with the device's own K ---------------------------------------
def _device_loop(lname, order):
    """(K list, obs, ctrls) of a closed-loop plan's problems taken in `order`."""
    L, d = E.LOOPS[lname], E.make_loop(lname)
    probs = [L["problems"][i] for i in order]
    cases = [_checked_case(case) for case, _ in probs]
    handles = [_handle(A, B) for A, B, _, _, _ in cases]
    sur = _handle(d["As"], d["Bs"])
    plan = _lib.LqrPlan(handles, L["no"], L["nu"])
    try:
        K, status = plan.gains([E.CASES[case]["horizon"] for case, _ in probs], np.array([c[2] for c in cases]),
                               np.array([c[3] for c in cases]), np.array([c[4] for c in cases]))
        assert np.all(status == 0)
        plan.set_loop([rule for _, rule in probs], d["goal"][order], d["lo"], d["hi"])
        obs, ctrls = plan.closed_loop(sur, [d["s0"][i] for i in order], d["sim0"][order], E.T_LOOP)
    finally:
        plan.close()
        for h in handles + [sur]:
            h.close()
    return K, obs, ctrls


@pytest.mark.parametrize("lname", list(E.LOOPS))
def test_closed_loop_against_long_double(lname):
    assert np.finfo(np.longdouble).eps < 2e-19
    L, d = E.LOOPS[lname], E.make_loop(lname)
    B = len(L["problems"])
    order = np.arange(B)
    K, obs, ctrls = _device_loop(lname, order)
    seen = np.zeros(3, dtype=bool)
    for i, (case, rule) in enumerate(L["problems"]):
        A, Bm = E.make_case(case)[:2]
        args = (A, Bm, K[i], rule, L["no"], d["goal"][i], d["s0"][i], d["sim0"][i], d["As"], d["Bs"], d["lo"], d["hi"],
                E.T_LOOP)
        o64, c64 = E.closed_loop(*args, dtype=np.float64)
        old, cld = E.closed_loop(*args, dtype=np.longdouble)
        seen |= np.array(E.clipping(c64, d["lo"], d["hi"]))
        for what, dev, f64, ld in (("obs", obs[i], o64, old), ("ctrls", ctrls[i], c64, cld)):
            host_err, err = E.rel_err(f64, ld), E.rel_err(dev, ld)
            print("%-8s %-20s %-5s host_err %.1e  device %.1e  tolerance %.1e" % (lname, case, what, host_err, err,
                                                                                  E.tolerance(host_err)))
            assert err <= E.tolerance(host_err), (lname, case, what, err, host_err)
    # a control on its upper bound at some step, one on its lower, one never clipped (bounds differ per control:
    # control 0 free, 1 bounded above only, 2 below only)
    assert L["nu"] < 3 or seen.all(), seen
    perm = order[::-1] if B < 3 else np.roll(order, 1)
    _, op, cp = _device_loop(lname, perm)
    assert np.array_equal(op, obs[perm]) and np.array_equal(cp, ctrls[perm])
