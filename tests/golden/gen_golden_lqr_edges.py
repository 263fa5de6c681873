#!/usr/bin/env python3
"""Expected gains of the LQR edge cases (tests/lqr_edge_cases.py), in extended precision.  CPU only:

    python tests/golden/gen_golden_lqr_edges.py

Writes ``tests/golden/lqr_edges.npz`` (data only).  Per case ``NAME``:
  K_NAME          the reference's recursion (lqr.py:15-47, its own association order) in numpy long double with a
                  hand-written Gauss-Jordan inverse, rounded to f64;
  host_err_NAME   max|lqr_gain_host - K| / max|K|: what the f64 host form loses, the tolerance's yardstick;
  checksum_NAME   exact sum and sum of squares of A, B, Q, R, F;
  exchanges_NAME  row exchanges of every solve in ``lqr_edge_cases.kernel_model``, the numpy model of the kernel.
The script asserts: long double is the 64-bit-mantissa format (eps < 2e-19); the long-double recursion agrees with
mpmath at 40 digits on one small pivoting case; every solve of every pivot* case exchanges rows at least once and no
solve of any other case does; the kernel model agrees with K within the tests' tolerance on every case; on the
closed-loop plans with three controls or more (the model's K, f64 restatement) a control reaches its upper bound, one
its lower, and one is never clipped.  Printed when the fixture was made (checksums left out here):

    n1_u1_o1_diag          exchanges per solve 0..0  host_err 5.6e-17  kernel model 7.6e-17  max|K| 8.41e-01
    n16_u1_o16_asym        exchanges per solve 0..0  host_err 3.2e-16  kernel model 3.9e-16  max|K| 2.32e-01
    n17_u2_o5_pivot: long double against mpmath at 40 digits 2.6e-19
    n17_u2_o5_pivot        exchanges per solve 1..1  host_err 5.4e-16  kernel model 3.3e-16  max|K| 1.05e-01
    n60_u4_o6_pivot_asym   exchanges per solve 2..2  host_err 1.2e-15  kernel model 1.6e-15  max|K| 1.98e-02
    n60_u5_o6_diag         exchanges per solve 0..0  host_err 1.9e-15  kernel model 2.4e-15  max|K| 3.88e-01
    n63_u16_o8_asym        exchanges per solve 0..0  host_err 1.4e-15  kernel model 1.8e-15  max|K| 1.96e-01
    n64_u16_o64_pivot      exchanges per solve 6..6  host_err 1.8e-15  kernel model 1.7e-15  max|K| 1.02e-01
    n65_u7_o5_asym         exchanges per solve 0..0  host_err 4.9e-15  kernel model 4.7e-15  max|K| 2.43e-01
    n127_u15_o9_pivot_asym exchanges per solve 5..6  host_err 1.8e-14  kernel model 4.7e-14  max|K| 7.18e-02
    n128_u16_o17_diag      exchanges per solve 0..0  host_err 2.0e-15  kernel model 2.8e-15  max|K| 1.49e-01
    n129_u3_o17_pivot      exchanges per solve 1..1  host_err 1.5e-15  kernel model 9.4e-16  max|K| 4.94e-02
    n192_u16_o6_asym       exchanges per solve 0..0  host_err 2.6e-15  kernel model 3.5e-15  max|K| 1.25e-01
    n193_u1_o6_diag        exchanges per solve 0..0  host_err 8.8e-16  kernel model 1.2e-15  max|K| 1.53e-01
    n240_u16_o17_pivot_asym exchanges per solve 4..6  host_err 1.9e-14  kernel model 1.6e-14  max|K| 3.42e-01
    n255_u15_o17_asym      exchanges per solve 0..0  host_err 5.2e-15  kernel model 7.7e-15  max|K| 1.55e-01
    n256_u16_o17_diag      exchanges per solve 0..0  host_err 3.2e-15  kernel model 3.5e-15  max|K| 1.20e-01
    n256_u16_o17_pivot     exchanges per solve 4..5  host_err 2.4e-15  kernel model 2.3e-15  max|K| 4.08e-02
    n256_u16_o256_asym     exchanges per solve 0..0  host_err 1.6e-15  kernel model 1.7e-15  max|K| 7.67e-02
    n256_u1_o1_diag        exchanges per solve 0..0  host_err 1.3e-15  kernel model 2.0e-15  max|K| 8.84e-02
    n17_u16_o17_diag       exchanges per solve 0..0  host_err 3.8e-16  kernel model 5.9e-16  max|K| 6.40e-01
    n5_u7_o5_pivot         exchanges per solve 1..1  host_err 1.3e-15  kernel model 1.6e-15  max|K| 1.46e-01
    loop o17_u16  n256_u16_o17_diag    rule 1  max|obs| 6.94e-01 max|ctrls| 1.38e-01  f64 restatement against long double: obs 2.3e-16 ctrls 7.8e-16  upper / lower / never clipped (True, True, True)
    loop o17_u16  n17_u16_o17_diag     rule 0  max|obs| 5.66e-01 max|ctrls| 1.70e-01  f64 restatement against long double: obs 2.4e-16 ctrls 4.2e-16  upper / lower / never clipped (True, True, True)
    loop o17_u16  n128_u16_o17_diag    rule 1  max|obs| 4.83e-01 max|ctrls| 9.97e-02  f64 restatement against long double: obs 3.4e-16 ctrls 8.3e-16  upper / lower / never clipped (True, True, True)
    loop o1_u1    n1_u1_o1_diag        rule 0  max|obs| 5.54e-01 max|ctrls| 3.52e-01  f64 restatement against long double: obs 1.6e-16 ctrls 2.4e-16  upper / lower / never clipped (False, False, True)
    loop o1_u1    n256_u1_o1_diag      rule 1  max|obs| 5.06e-01 max|ctrls| 1.43e-01  f64 restatement against long double: obs 2.9e-16 ctrls 3.9e-16  upper / lower / never clipped (False, False, True)
    loop o5_u7    n65_u7_o5_asym       rule 1  max|obs| 3.00e+01 max|ctrls| 1.34e+00  f64 restatement against long double: obs 1.8e-16 ctrls 4.6e-16  upper / lower / never clipped (True, True, True)
    loop o5_u7    n5_u7_o5_pivot       rule 0  max|obs| 1.01e+00 max|ctrls| 1.70e-01  f64 restatement against long double: obs 3.8e-16 ctrls 2.9e-16  upper / lower / never clipped (False, False, True)
    wrote lqr_edges.npz 254.9 KB
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lqr_edge_cases as E                                    # noqa: E402
from autompc_amd.control.lqr import lqr_gain_host            # noqa: E402

MP_CASE = "n17_u2_o5_pivot"


def mpmath_gain(A, B, Q, R, F, horizon, digits=40):
    """The same recursion in mpmath (its own LU inverse)."""
    import mpmath as mp
    mp.mp.dps = digits
    n = A.shape[0]
    A, B, R = mp.matrix(A.tolist()), mp.matrix(B.tolist()), mp.matrix(R.tolist())
    Qp, P = mp.matrix(E.pad(Q, n).tolist()), mp.matrix(E.pad(F, n).tolist())
    for _ in range(horizon + 1):
        P = A.T * P * A - (A.T * P * B) * mp.inverse(R + B.T * P * B) * (B.T * P * A) + Qp
    K = -mp.inverse(R + B.T * P * B) * B.T * P * A
    return np.array([[mp.nstr(K[i, j], 25) for j in range(K.cols)] for i in range(K.rows)], dtype=np.longdouble)


def gen():
    assert np.finfo(np.longdouble).eps < 2e-19, "long double is not the x87 extended format here"
    out = {}
    for name, c in E.CASES.items():
        A, B, Q, R, F = E.make_case(name)
        K = E.riccati(A, B, Q, R, F, c["horizon"])
        assert np.all(np.isfinite(K)), name
        if name == MP_CASE:
            mp_err = E.rel_err(K, mpmath_gain(A, B, Q, R, F, c["horizon"]))
            assert mp_err < 1e-17, mp_err
            print("    %s: long double against mpmath at 40 digits %.1e" % (name, mp_err))
        host_err = E.rel_err(lqr_gain_host(A, B, Q, R, F, c["horizon"]), K)
        Km, status, counts = E.kernel_model(A, B, Q, R, F, c["horizon"])
        model_err = E.rel_err(Km, K)
        assert status == 0 and model_err <= E.tolerance(host_err), (name, model_err, host_err)
        if E.pivoting(name):
            assert min(counts) >= 1, (name, counts)
        else:
            assert max(counts) == 0, (name, counts)
        cs = E.checksum((A, B, Q, R, F))
        out.update({"K_" + name: K.astype(np.float64), "host_err_" + name: host_err, "checksum_" + name: cs,
                    "exchanges_" + name: np.array(counts, dtype=np.int32)})
        print("    %-22s exchanges per solve %d..%d  host_err %.1e  kernel model %.1e  max|K| %.2e  checksum A %.17g "
              "%.17g B %.17g %.17g" % (name, min(counts), max(counts), host_err, model_err, np.abs(K).max(),
                                       cs[0, 0], cs[0, 1], cs[1, 0], cs[1, 1]))
    for lname, L in E.LOOPS.items():
        d = E.make_loop(lname)
        seen = np.zeros(3, dtype=bool)
        for i, (case, rule) in enumerate(L["problems"]):
            A, B, Q, R, F = E.make_case(case)
            K = E.kernel_model(A, B, Q, R, F, E.CASES[case]["horizon"])[0]
            args = (A, B, K, rule, L["no"], d["goal"][i], d["s0"][i], d["sim0"][i], d["As"], d["Bs"], d["lo"], d["hi"],
                    E.T_LOOP)
            o64, c64 = E.closed_loop(*args, dtype=np.float64)
            old, cld = E.closed_loop(*args, dtype=np.longdouble)
            assert np.all(np.isfinite(o64)) and np.all(np.isfinite(c64)), (lname, case)
            clip = E.clipping(c64, d["lo"], d["hi"])
            seen |= np.array(clip)
            print("    loop %-8s %-20s rule %d  max|obs| %.2e max|ctrls| %.2e  f64 restatement against long double: obs "
                  "%.1e ctrls %.1e  upper / lower / never clipped %s" % (
                      lname, case, rule, np.abs(o64).max(), np.abs(c64).max(), E.rel_err(o64, old),
                      E.rel_err(c64, cld), clip))
        assert L["nu"] < 3 or seen.all(), (lname, seen)
    path = os.path.join(HERE, "lqr_edges.npz")
    np.savez_compressed(path, **out)
    print("    wrote lqr_edges.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    gen()
