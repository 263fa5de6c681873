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
100 x the largest error_form_error over all cases is ``sysid.stable_fit.TIE``.  Printed when the goldens were made:

    n2       n  2 rows   33  rho 1.0657 -> 1.0000  iterations 29 trials  95  host_err 8.7e-16  margin 4.4e-08  gram_err 3.0e-16  error form 2.5e-14 (all evaluations 2.5e-14)  roundoff_response 1.1e-15
    n12      n 12 rows  234  rho 1.0439 -> 0.9978  iterations 29 trials  82  host_err 2.4e-13  margin 1.7e-05  gram_err 5.8e-13  error form 5.4e-15 (all evaluations 9.5e-01)  roundoff_response 7.0e-13
    n51      n 51 rows 1980  rho 1.0053 -> 0.9989  iterations 29 trials  68  host_err 1.1e-10  margin 4.8e-06  gram_err 1.1e-10  error form 9.2e-16 (all evaluations 9.1e-01)  roundoff_response 8.1e-14
    n64      n 64 rows  660  rho 1.6330 -> 0.9968  iterations 29 trials  69  host_err 7.1e-12  margin 3.3e-06  gram_err 2.5e-11  error form 3.6e-15 (all evaluations 7.8e-01)  roundoff_response 2.5e-11
    inactive n  6 rows  156  rho 0.9561 -> 0.9560  iterations 29 trials  91  host_err 6.6e-07  margin 2.4e-09  gram_err 6.6e-07  error form 3.5e-14 (all evaluations 3.5e-14)  roundoff_response 9.3e-15
    dup      n  6 rows  145  rho 1.0380 -> 0.9830  iterations 29 trials  68  host_err 2.0e-02  margin 9.1e-05  Gram route: status 1
    largest error-form difference 3.47e-14 -> ERROR_FORM_ERROR; TIE = 100 x that
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
from stablefit_cases import CASES, FITTED, basis, make_data, rel_err   # noqa: E402


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


def perturbation(seed):
    rng = np.random.default_rng(seed)

    def perturb(Gm, Q, yy):
        Z = rng.uniform(-1.0, 1.0, size=Gm.shape)
        Z = np.triu(Z) + np.triu(Z, 1).T
        return (Gm * (1.0 + 2.0 ** -52 * Z), Q * (1.0 + 2.0 ** -52 * rng.uniform(-1.0, 1.0, size=Q.shape)),
                yy * (1.0 + 2.0 ** -52 * rng.uniform(-1.0, 1.0, size=yy.shape)))
    return perturb


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
    if name in FITTED:
        assert (stats["iterations"], stats["trials"]) == (its, trials), (name, stats, its, trials)
        assert ref_margin > SF.TIE and stats["margin"] > SF.TIE, (name, ref_margin, stats["margin"])
    out = dict(traj_len=lens, obs=obs, ctrls=ctrls, A=A, B=Bc, error=error, iterations=its, trials=trials,
               host_err=host_err, margin=ref_margin, host_margin=stats["margin"], rho=np.max(np.abs(np.linalg.eigvals(A))),
               rho_lstsq=np.max(np.abs(np.linalg.eigvals((Y @ np.linalg.pinv(np.vstack([Xs, Xu])))[:, :n]))))
    line = "    %-8s n %2d rows %4d  rho %.4f -> %.4f  iterations %2d trials %3d  host_err %.1e  margin %.1e" % (
        name, n, Xs.shape[1], out["rho_lstsq"], out["rho"], its, trials, host_err, ref_margin)
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
        pert = SF.stable_fit_host(lens, obs, ctrls, [b], perturb=perturbation(CASES[name]["seed"]))
        assert pert[1][0] == 0, name
        out.update(gram_err=rel_err(coeffs[0], refc), error_form_error=form,
                   roundoff_response=rel_err(pert[0][0], coeffs[0]))
        assert (git[0], gtr[0]) == (its, trials), (name, git, gtr)
        line += "  gram_err %.1e  error form %.1e (all evaluations %.1e)  roundoff_response %.1e" % (
            out["gram_err"], form, form_all, out["roundoff_response"])
    else:
        out.update(gram_err=np.nan, error_form_error=0.0, roundoff_response=0.0)
        line += "  Gram route: status %d" % status[0]
    assert (status[0] == 0) == (name in FITTED), (name, status)
    print(line)
    G.save("stablefit_" + name, **out)
    return form


def gen():
    worst = max(gen_case(name) for name in CASES)
    print("    largest error-form difference %.2e -> ERROR_FORM_ERROR; TIE = 100 x that" % worst)


if __name__ == "__main__":
    gen()
