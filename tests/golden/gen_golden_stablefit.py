#!/usr/bin/env python3
"""Golden vectors of the stable Koopman fits, from the REAL reference (williamedwards/autompc).

Run in the build container only (needs the reference checkout that gen_golden.py installs, with its
``scipy.linalg.pinv2`` alias):

    python tests/golden/gen_golden_stablefit.py

Writes ``tests/golden/stablefit_*.npz`` (data only), one per case of ``tests/stablefit_cases.py``: the training data
(``traj_len``, concatenated ``obs`` / ``ctrls``: ``stablefit_cases.make_data``) and what the reference's own
``stabilize_discrete(Xs, Xu, Y)`` makes of the lifted data -- ``A``, ``B`` (its ``Bcon``), ``error`` -- with the outer
iterations it ran (``iterations``: calls of ``math.sqrt`` through a counting stand-in for the module's ``math``, one
per loop body) and its line-search trials (``trials``: calls of its ``gradients`` through a wrapper, less one for the
start and one per iteration).  The reference is not edited; its prints are swallowed.  The script asserts that the
reference's result is real and finite.

Per case it also stores and prints
  host_err           max|d[A | B]| / max|[A | B]| of ``stable_fit.stabilize_host`` against the reference;
  gram_err           the same for ``stable_fit.stable_fit_host`` (not a tolerance: reported);
  error_form_error   the largest |e_Gram - e_data| / e_data over the error evaluations of ``stable_fit_host`` with
                     e_data <= 10 x the error that evaluation is compared with (the start included), the data-form
                     error evaluated at the same iterate.  e0^2 comes from the Schur complement sum yy - sum W0 o Q',
                     so this figure includes its cancellation.  The figure over all evaluations is printed next to
                     it: the over-long first trials of a line search clip S at 1e-15, and there the data form's own
                     inv(S) is rounding noise.  The script asserts that at every evaluation left out BOTH forms'
                     errors exceed 10 x the error they are compared with: no such decision can turn;
  margin             the smallest decision margin |e_next - e| / e of the REFERENCE's own run, from the errors its
                     ``gradients`` returned (asserted above ``stable_fit.TIE``); host_margin: the restatement's;
  roundoff_response  max|d[A | B]| / max|[A | B]| of ``stable_fit_host`` when every Gram entry is multiplied by
                     1 + 2^-52 z, z seeded uniform in [-1, 1] (symmetrically): what the case makes of one rounding.
100 x the largest error_form_error over all cases (the sweep below included) is ``sysid.stable_fit.TIE``.  Printed
when the goldens were made:

    n2       n  2 rows   33  rho 1.0657 -> 1.0000  iterations 29 trials  95  host_err 8.7e-16  margin 4.4e-08  gram_err 3.0e-16  error form 2.5e-14 (all evaluations 2.5e-14)  roundoff_response 1.1e-15
    n12      n 12 rows  234  rho 1.0439 -> 0.9978  iterations 29 trials  82  host_err 2.4e-13  margin 1.7e-05  gram_err 5.8e-13  error form 5.4e-15 (all evaluations 9.5e-01)  roundoff_response 7.0e-13
    n51      n 51 rows 1980  rho 1.0053 -> 0.9989  iterations 29 trials  68  host_err 1.1e-10  margin 4.8e-06  gram_err 1.1e-10  error form 9.2e-16 (all evaluations 9.1e-01)  roundoff_response 8.1e-14
    n64      n 64 rows  660  rho 1.6330 -> 0.9968  iterations 29 trials  69  host_err 7.1e-12  margin 3.3e-06  gram_err 2.5e-11  error form 3.6e-15 (all evaluations 7.8e-01)  roundoff_response 2.5e-11
    inactive n  6 rows  156  rho 0.9561 -> 0.9560  iterations 29 trials  91  host_err 6.6e-07  margin 2.4e-09  gram_err 6.6e-07  error form 3.5e-14 (all evaluations 3.5e-14)  roundoff_response 9.3e-15
    dup      n  6 rows  145  rho 1.0380 -> 0.9830  iterations 29 trials  68  host_err 2.0e-02  margin 9.1e-05  Gram route: status 1
    largest error-form difference 3.47e-14

``python tests/golden/gen_golden_stablefit.py sweep [names]`` writes the goldens of ``stablefit_cases.SWEEP`` alone
(``stablefit_sweep_*.npz``): the size sweep and its ragged-rows case, through the same ``gen_case`` with the same fields
and assertions.  A case on which the reference fails one of them takes the next seed, recorded in the table (n = 2 ties
at the rule's seeds; ``sweep_ragged`` at seed 6105 makes the reference's own ``inv(S)`` raise "Singular matrix" in a
line search).  The cases of one lifted state tie in every run (``gen_tied``: data, the host forms' status and margins;
no reference comparison).  Their error-form differences exceed the first six cases': ``ERROR_FORM_ERROR`` is the
largest over BOTH tables, 1.2e-12 in ``sweep_ragged`` (rounded up to 1.3e-12), and TIE = 100 x that.  Printed:

    sweep_n1_u1   n  1 rows   44  Gram route: status 2, margin 0.0e+00 (iterations 29 trials 176); stabilize_host margin 0.0e+00
    sweep_n2_u1   n  2 rows   55  rho 1.0178 -> 1.0000  iterations 29 trials  85  host_err 1.1e-15  margin 1.8e-05  gram_err 5.2e-15  error form 1.8e-13 (all evaluations 1.8e-13)  roundoff_response 9.9e-16
    sweep_n3_u1   n  3 rows   55  rho 1.0761 -> 1.0000  iterations 29 trials  70  host_err 3.3e-12  margin 2.3e-05  gram_err 3.3e-12  error form 8.1e-14 (all evaluations 8.1e-14)  roundoff_response 3.8e-14
    sweep_n4_u1   n  4 rows   66  rho 1.0571 -> 1.0000  iterations 29 trials  62  host_err 8.7e-10  margin 4.2e-04  gram_err 7.9e-10  error form 1.4e-13 (all evaluations 1.4e-13)  roundoff_response 1.3e-10
    sweep_n5_u1   n  5 rows   77  rho 1.0635 -> 1.0000  iterations 29 trials  60  host_err 9.1e-12  margin 1.2e-04  gram_err 9.1e-12  error form 6.6e-14 (all evaluations 6.6e-14)  roundoff_response 1.7e-14
    sweep_n15_u1  n 15 rows  154  rho 1.0477 -> 0.9999  iterations 29 trials  60  host_err 1.5e-10  margin 6.5e-05  gram_err 1.5e-10  error form 3.2e-14 (all evaluations 2.1e-02)  roundoff_response 7.0e-12
    sweep_n16_u1  n 16 rows  165  rho 1.0608 -> 0.9997  iterations 29 trials  62  host_err 7.8e-12  margin 4.0e-05  gram_err 6.9e-12  error form 2.9e-14 (all evaluations 7.9e-02)  roundoff_response 1.3e-13
    sweep_n17_u1  n 17 rows  165  rho 1.0586 -> 0.9997  iterations 29 trials  61  host_err 8.0e-11  margin 6.7e-04  gram_err 7.8e-11  error form 1.0e-13 (all evaluations 3.8e-02)  roundoff_response 3.5e-12
    sweep_n31_u1  n 31 rows  286  rho 1.0453 -> 0.9996  iterations 29 trials  62  host_err 4.2e-11  margin 4.7e-04  gram_err 4.3e-11  error form 4.5e-14 (all evaluations 1.9e-01)  roundoff_response 8.6e-13
    sweep_n32_u1  n 32 rows  286  rho 1.0425 -> 0.9988  iterations 29 trials  63  host_err 5.4e-10  margin 1.6e-03  gram_err 5.6e-10  error form 2.7e-14 (all evaluations 8.8e-02)  roundoff_response 3.9e-12
    sweep_n33_u1  n 33 rows  297  rho 1.0345 -> 0.9999  iterations 29 trials  62  host_err 2.9e-11  margin 6.7e-04  gram_err 2.8e-11  error form 1.1e-14 (all evaluations 4.4e-02)  roundoff_response 2.1e-12
    sweep_n47_u1  n 47 rows  407  rho 1.0551 -> 0.9994  iterations 29 trials  64  host_err 1.1e-11  margin 8.7e-04  gram_err 1.0e-11  error form 2.8e-14 (all evaluations 1.0e-01)  roundoff_response 4.4e-13
    sweep_n48_u1  n 48 rows  418  rho 1.0464 -> 0.9986  iterations 29 trials  64  host_err 1.3e-12  margin 3.4e-04  gram_err 1.3e-12  error form 1.1e-14 (all evaluations 8.8e-02)  roundoff_response 1.1e-14
    sweep_n49_u1  n 49 rows  429  rho 1.0569 -> 0.9987  iterations 29 trials  64  host_err 1.9e-12  margin 3.1e-06  gram_err 1.9e-12  error form 1.1e-14 (all evaluations 8.2e-02)  roundoff_response 7.1e-14
    sweep_n62_u1  n 62 rows  528  rho 1.0497 -> 0.9982  iterations 29 trials  64  host_err 1.5e-10  margin 9.1e-04  gram_err 1.5e-10  error form 5.9e-14 (all evaluations 2.1e-01)  roundoff_response 3.7e-12
    sweep_n63_u1  n 63 rows  539  rho 1.0436 -> 0.9983  iterations 29 trials  66  host_err 3.1e-11  margin 3.2e-04  gram_err 2.9e-11  error form 2.6e-14 (all evaluations 2.9e-01)  roundoff_response 6.4e-13
    sweep_n64_u1  n 64 rows  550  rho 1.0477 -> 0.9985  iterations 29 trials  64  host_err 3.1e-12  margin 4.9e-04  gram_err 3.0e-12  error form 2.8e-14 (all evaluations 2.4e-01)  roundoff_response 1.3e-14
    sweep_n1_u16  n  1 rows  165  Gram route: status 2, margin 5.3e-14 (iterations 29 trials 156); stabilize_host margin 5.4e-14
    sweep_n2_u16  n  2 rows  165  rho 1.0125 -> 1.0000  iterations 29 trials  90  host_err 3.6e-16  margin 8.5e-07  gram_err 1.3e-15  error form 8.0e-13 (all evaluations 8.0e-13)  roundoff_response 3.6e-16
    sweep_n3_u16  n  3 rows  176  rho 1.0496 -> 1.0000  iterations 29 trials 109  host_err 2.3e-12  margin 6.9e-07  gram_err 2.3e-12  error form 1.1e-13 (all evaluations 3.1e-04)  roundoff_response 1.4e-15
    sweep_n4_u16  n  4 rows  187  rho 1.0430 -> 1.0000  iterations 29 trials  60  host_err 1.5e-12  margin 9.1e-05  gram_err 1.5e-12  error form 1.9e-14 (all evaluations 1.1e-01)  roundoff_response 3.2e-14
    sweep_n5_u16  n  5 rows  198  rho 1.0495 -> 1.0000  iterations 29 trials  74  host_err 7.8e-13  margin 1.7e-05  gram_err 7.8e-13  error form 7.3e-14 (all evaluations 3.7e-02)  roundoff_response 4.4e-15
    sweep_n15_u16 n 15 rows  275  rho 1.0368 -> 1.0000  iterations 29 trials  62  host_err 1.3e-12  margin 7.6e-05  gram_err 1.3e-12  error form 2.0e-13 (all evaluations 1.6e-01)  roundoff_response 1.6e-14
    sweep_n16_u16 n 16 rows  286  rho 1.0331 -> 1.0000  iterations 29 trials  63  host_err 6.8e-13  margin 1.9e-05  gram_err 6.8e-13  error form 4.8e-14 (all evaluations 6.2e-02)  roundoff_response 1.8e-14
    sweep_n17_u16 n 17 rows  286  rho 1.0402 -> 1.0000  iterations 29 trials  63  host_err 3.8e-12  margin 3.9e-05  gram_err 3.9e-12  error form 2.0e-13 (all evaluations 1.5e-01)  roundoff_response 1.4e-13
    sweep_n31_u16 n 31 rows  407  rho 1.0426 -> 1.0000  iterations 29 trials  64  host_err 1.4e-12  margin 1.3e-04  gram_err 1.4e-12  error form 5.8e-14 (all evaluations 2.5e-01)  roundoff_response 2.7e-14
    sweep_n32_u16 n 32 rows  407  rho 1.0357 -> 1.0000  iterations 29 trials  64  host_err 2.8e-12  margin 1.3e-04  gram_err 2.8e-12  error form 8.6e-14 (all evaluations 3.5e-01)  roundoff_response 2.9e-14
    sweep_n33_u16 n 33 rows  418  rho 1.0340 -> 1.0000  iterations 29 trials  64  host_err 6.2e-12  margin 2.4e-04  gram_err 5.6e-12  error form 1.2e-14 (all evaluations 4.0e-01)  roundoff_response 9.8e-14
    sweep_n47_u16 n 47 rows  528  rho 1.0409 -> 1.0000  iterations 29 trials  65  host_err 5.9e-10  margin 2.9e-04  gram_err 5.7e-10  error form 1.5e-14 (all evaluations 6.9e-01)  roundoff_response 8.3e-12
    sweep_n48_u16 n 48 rows  539  rho 1.0304 -> 1.0000  iterations 29 trials  66  host_err 4.0e-12  margin 5.0e-05  gram_err 4.9e-12  error form 1.0e-14 (all evaluations 8.5e-01)  roundoff_response 1.6e-12
    sweep_n49_u16 n 49 rows  550  rho 1.0409 -> 1.0000  iterations 29 trials  65  host_err 3.5e-11  margin 1.8e-05  gram_err 3.5e-11  error form 7.5e-15 (all evaluations 8.0e-01)  roundoff_response 4.2e-13
    sweep_n62_u16 n 62 rows  649  rho 1.0336 -> 0.9997  iterations 29 trials  67  host_err 5.1e-12  margin 4.6e-04  gram_err 5.0e-12  error form 1.1e-13 (all evaluations 9.4e-01)  roundoff_response 5.4e-14
    sweep_n63_u16 n 63 rows  660  rho 1.0386 -> 0.9999  iterations 29 trials  67  host_err 7.4e-11  margin 9.6e-05  gram_err 7.4e-11  error form 2.3e-14 (all evaluations 8.6e-01)  roundoff_response 3.2e-13
    sweep_n64_u16 n 64 rows  671  rho 1.0357 -> 1.0000  iterations 29 trials  66  host_err 6.1e-11  margin 6.8e-04  gram_err 6.3e-11  error form 1.1e-14 (all evaluations 9.1e-01)  roundoff_response 1.4e-12
    sweep_ragged  n  5 rows  578  rho 1.0101 -> 1.0000  iterations 29 trials  80  host_err 8.2e-11  margin 1.7e-05  gram_err 8.1e-11  error form 1.2e-12 (all evaluations 2.4e+01)  roundoff_response 2.4e-14
    largest error-form difference of the sweep 1.20e-12 -> ERROR_FORM_ERROR; TIE = 100 x that
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G                                        # noqa: E402  (installs the reference)
import autompc.sysid.stable_koopman as ref                    # noqa: E402

from autompc_amd.sysid import stable_fit as SF                # noqa: E402
from stablefit_cases import (CASES, FITTED, SWEEP, SWEEP_FITTED, SWEEP_TIED, basis, case, make_data,   # noqa: E402
                             perturbation, rel_err)


FAR = 10.0          # error evaluations above FAR x the current error are left out of error_form_error


class CountingMath:
    """The module's ``math`` with sqrt counted: stabilize_discrete takes one square root per outer iteration."""
    calls = 0
    inf = math.inf

    @classmethod
    def sqrt(cls, x):
        cls.calls += 1
        return math.sqrt(x)


def run_reference(Xs, Xu, Y):
    """(A, Bcon, error, iterations, trials, smallest decision margin) of the reference's own run."""
    calls = []                                                # (error returned, square roots taken so far)
    real = ref.gradients

    def counted(*a):
        out = real(*a)
        calls.append((float(out[0]), CountingMath.calls))
        return out
    ref.gradients, ref.math = counted, CountingMath
    CountingMath.calls = 0
    try:
        Kd, S, U, B, Bcon, error = G.quiet(ref.stabilize_discrete, Xs, Xu, Y)
    finally:
        ref.gradients, ref.math = real, math
    its = CountingMath.calls
    # iteration k's calls are those made after k - 1 square roots: the gradient at the current iterate (its error is
    # the one the trials are compared with), then the trials; the very first call is the start's error
    margin = math.inf
    for k in range(its):
        es = [e for e, roots in calls[1:] if roots == k]
        margin = min([margin] + [abs(e - es[0]) / es[0] for e in es[1:]])
    return Kd, Bcon, float(error), its, len(calls) - 1 - its, margin


def gen_case(name):
    lens, obs, ctrls = make_data(name)
    b = basis(name)
    Xs, Xu, Y = SF.koopman_rows(lens, obs, ctrls, b)
    n = Xs.shape[0]
    A, Bc, error, its, trials, ref_margin = run_reference(Xs, Xu, Y)
    assert np.isrealobj(A) and np.isrealobj(Bc) and np.all(np.isfinite(A)) and np.all(np.isfinite(Bc)), name
    refc = np.hstack([A, Bc])
    stats = {}
    hA, hB, herr = SF.stabilize_host(Xs, Xu, Y, stats)
    host_err = rel_err(np.hstack([hA, hB]), refc)
    fitted = name in FITTED or name in SWEEP_FITTED
    if fitted:
        assert (stats["iterations"], stats["trials"]) == (its, trials), (name, stats, its, trials)
        assert ref_margin > SF.TIE and stats["margin"] > SF.TIE, (name, ref_margin, stats["margin"])
    out = dict(traj_len=lens, obs=obs, ctrls=ctrls, A=A, B=Bc, error=error, iterations=its, trials=trials,
               host_err=host_err, margin=ref_margin, host_margin=stats["margin"], rho=np.max(np.abs(np.linalg.eigvals(A))),
               rho_lstsq=np.max(np.abs(np.linalg.eigvals((Y @ np.linalg.pinv(np.vstack([Xs, Xu])))[:, :n]))))
    line = "    %-*s n %2d rows %4d  rho %.4f -> %.4f  iterations %2d trials %3d  host_err %.1e  margin %.1e" % (
        13 if name in SWEEP else 8, name, n, Xs.shape[1], out["rho_lstsq"], out["rho"], its, trials, host_err, ref_margin)
    log = []
    coeffs, status, gerr, git, gtr, gmar = SF.stable_fit_host(lens, obs, ctrls, [b], log=log)
    form = 0.0
    if status[0] == 0:
        ops = SF._DataOps(Xs, Xu, Y)
        pairs = [(e, ops.error(it), cur) for e, it, cur in log]
        form_all = max(abs(e - de) / de for e, de, _ in pairs)
        near = [cur is None or de <= FAR * cur for _, de, cur in pairs]
        form = max(abs(e - de) / de for (e, de, _), nr in zip(pairs, near) if nr)
        # what is left out cannot turn a decision: there BOTH forms' errors are more than FAR x the error they are
        # compared with (a trial is accepted only at or below it)
        assert all(min(e, de) > FAR * cur for (e, de, cur), nr in zip(pairs, near) if not nr), name
        pert = SF.stable_fit_host(lens, obs, ctrls, [b], perturb=perturbation(case(name)["seed"]))
        assert pert[1][0] == 0, name
        out.update(gram_err=rel_err(coeffs[0], refc), error_form_error=form,
                   roundoff_response=rel_err(pert[0][0], coeffs[0]))
        assert (git[0], gtr[0]) == (its, trials), (name, git, gtr)
        line += "  gram_err %.1e  error form %.1e (all evaluations %.1e)  roundoff_response %.1e" % (
            out["gram_err"], form, form_all, out["roundoff_response"])
    else:
        out.update(gram_err=np.nan, error_form_error=0.0, roundoff_response=0.0)
        line += "  Gram route: status %d" % status[0]
    assert (status[0] == 0) == fitted, (name, status)
    print(line)
    G.save("stablefit_" + name, **out)
    return form


def gen_tied(name):
    """A sweep case of one lifted state: every run ties (status 2), so there is no reference comparison to make.
    Data only, with the host forms' status and margin."""
    lens, obs, ctrls = make_data(name)
    b = basis(name)
    stats = {}
    SF.stabilize_host(*SF.koopman_rows(lens, obs, ctrls, b), stats)
    _, status, _, git, gtr, gmar = SF.stable_fit_host(lens, obs, ctrls, [b])
    assert status[0] == 2 and gmar[0] <= SF.TIE and stats["margin"] <= SF.TIE, (name, status, gmar, stats)
    print("    %-13s n %2d rows %4d  Gram route: status %d, margin %.1e (iterations %d trials %d); stabilize_host margin "
          "%.1e" % (name, case(name)["no"], len(obs) - len(lens), status[0], gmar[0], git[0], gtr[0], stats["margin"]))
    G.save("stablefit_" + name, traj_len=lens, obs=obs, ctrls=ctrls, status=status[0], gram_margin=gmar[0],
           host_margin=stats["margin"])


def gen():
    worst = max(gen_case(name) for name in CASES)
    print("    largest error-form difference %.2e" % worst)


def gen_sweep(names=None):
    """The size sweep and the ragged-rows case (stablefit_cases.SWEEP): the same fields, the same assertions."""
    names = list(SWEEP) if names is None else names
    for name in names:
        if name in SWEEP_TIED:
            gen_tied(name)
    worst = max(gen_case(name) for name in names if name in SWEEP_FITTED)
    print("    largest error-form difference of the sweep %.2e -> ERROR_FORM_ERROR; TIE = 100 x that" % worst)


if __name__ == "__main__":
    if sys.argv[1:2] == ["sweep"]:
        gen_sweep(sys.argv[2:] or None)
    else:
        gen()
