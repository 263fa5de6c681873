#!/usr/bin/env python3
"""Golden vectors of the lasso Koopman fits, from the REAL reference (williamedwards/autompc).

Run in the build container only (needs the reference checkout that gen_golden.py installs):

    python tests/golden/gen_golden_lassofit.py

Writes ``tests/golden/lassofit_*.npz`` (data only), one per case of ``tests/lassofit_cases.py``: the training data
(``traj_len``, concatenated ``obs`` / ``ctrls``, the dynamics of gen_golden_linfit.train_trajs), the case's ``alphas``
and, per alpha k, what the reference's own ``Koopman(method="lasso").train`` makes of the data -- ``A_<k>``, ``B_<k>``
-- with sklearn's ``n_iter_`` of every target (``n_iter_<k>``, recorded from the ``Lasso`` object that ``train``
creates).  The reference builds its basis functions in its constructor; a case whose basis the constructor cannot
express (the documented, duplicate-free one) gets ``basis_funcs`` set to that list before ``train`` is called.

Per case and alpha the script prints the error of ``lasso_fit_host`` against the reference, max|dcoef| / max|coef|
(stored as ``host_err``, the largest of the case), whether the sweep counts equal ``n_iter_``, and the largest
``|gap_Gram - gap_residual| / tol_t`` over every gap check (sklearn's residual-form gap evaluated in numpy at the same
``w``): 100 x the largest of those over all cases is ``sysid.lasso_fit.TIE``; the two margins are the smallest gap margin
and the smallest sweep-test margin (``RATIO_TIE``).  Printed when the goldens were made:

    n13    alpha 100    err 0.0e+00  sweeps    1..   1  gap form 5.2e-12  margins 1.0e+00 inf
    n13    alpha 1      err 2.0e-15  sweeps    1..   4  gap form 7.4e-12  margins 1.0e+00 1.0e+00
    n13    alpha 0.01   err 2.0e-12  sweeps    5..1000  gap form 6.0e-11  margins 8.6e-02 1.2e-03
    n13    alpha 1e-06  err 3.3e-12  sweeps 1000..1000  gap form 9.3e-09  margins 7.5e-02 2.3e-04
    dup    alpha 0.1    err 1.8e-14  sweeps    3..  59  gap form 6.7e-12  margins 3.2e-01 1.4e-02
    dup    alpha 1e-05  err 6.2e-14  sweeps   57..1000  gap form 2.4e-05  margins 9.0e-03 1.0e-02
    n74    alpha 0.1    err 6.7e-14  sweeps    8..  60  gap form 3.0e-11  margins 3.1e-02 2.1e-03
    big    alpha 1      err 6.9e-14  sweeps    2..  76  gap form 8.9e-11  margins 3.9e-03 1.5e-04
    zero   alpha 0.001  err 1.3e-14  sweeps    7..  10  gap form 9.7e-11  margins 2.7e-01 4.2e-02
    const  alpha 0.001  status 1
    (sweeps equal sklearn's n_iter_ for every target of every line)
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G                                        # noqa: E402  (installs the reference)
import autompc.sysid.koopman as ref_koopman                   # noqa: E402
from gen_golden_linfit import train_trajs                     # noqa: E402

from autompc_amd.sysid import lasso_fit as LS                 # noqa: E402
from autompc_amd.sysid.linear_fit import koopman_design       # noqa: E402
from lassofit_cases import CASES, basis, rel_err              # noqa: E402

FUNCS = {0: lambda p: (lambda x: x), 1: lambda p: (lambda x: x ** int(p)), 2: lambda p: (lambda x: np.sin(p * x)),
         3: lambda p: (lambda x: np.cos(p * x))}


class RecordingLasso(ref_koopman.Lasso):
    """sklearn's Lasso, keeping the last fitted object so that n_iter_ can be read after train()."""
    last = None

    def fit(self, *a, **k):
        RecordingLasso.last = self
        return super().fit(*a, **k)


def residual_gap(F, y, w, alpha):
    """sklearn's duality gap of one target in its own residual form (centred data)."""
    R = y - F @ w
    XtA = F.T @ R
    dn = np.max(np.abs(XtA))
    r2 = R @ R
    if dn > alpha:
        c = alpha / dn
        gap = 0.5 * (r2 + r2 * c * c)
    else:
        c, gap = 1.0, r2
    return gap + alpha * np.sum(np.abs(w)) - c * (R @ y)


def gen_case(name):
    c = CASES[name]
    system = G.make_system(c["no"], c["nu"])
    trajs = train_trajs(system, c["lengths"], c["seed"])
    if c["hold"] is not None:
        for t in trajs:
            t.ctrls[:, c["hold"][0]] = c["hold"][1]
    lens = np.array([len(t) for t in trajs], dtype=np.int32)
    obs = np.concatenate([np.asarray(t.obs) for t in trajs])
    ctrls = np.concatenate([np.asarray(t.ctrls) for t in trajs])
    out = dict(traj_len=lens, obs=obs, ctrls=ctrls, alphas=np.array(c["alphas"]))
    kinds, params = basis(name)
    kw = {k: v for k, v in c["koopman"].items() if k != "strict_reference"}
    F, Y = koopman_design(lens, obs, ctrls, (kinds, params))
    Fc, Yc = F - F.mean(0), Y - Y.mean(0)
    worst, worst_gap = 0.0, 0.0
    ref_koopman.Lasso = RecordingLasso
    for k, alpha in enumerate(c["alphas"]):
        m = G.quiet(ref_koopman.Koopman, system, method="lasso", lasso_alpha=alpha, product_terms="false", **kw)
        if not c["koopman"].get("strict_reference", True):
            m.basis_funcs = [FUNCS[int(kd)](float(p)) for kd, p in zip(kinds, params)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                   # ConvergenceWarning at the sweep cap
            G.quiet(m.train, trajs)
        n_iter = np.atleast_1d(RecordingLasso.last.n_iter_).astype(np.int32)
        out["A_%d" % k], out["B_%d" % k], out["n_iter_%d" % k] = np.asarray(m.A), np.asarray(m.B), n_iter
        log = []
        coeffs, status, margin, sweeps, per = LS.lasso_fit_host(lens, obs, ctrls, [(kinds, params)], [(0, alpha)],
                                                                per_target=True, gap_log=log)
        line = "%-6s alpha %-6g status %d" % (name, alpha, status[0])
        if status[0] != 1:
            err = rel_err(coeffs[0], np.hstack([m.A, m.B]))
            gap_err = max([abs(g - residual_gap(Fc, Yc[:, t], w, alpha * len(F))) / tol
                           for _, t, w, g, tol in log if tol > 0] or [0.0])
            worst, worst_gap = max(worst, err), max(worst_gap, gap_err)
            line += "  err %.1e  sweeps %4d..%4d equal %s  gap form %.1e  margins %.1e %.1e" % (
                err, per[0].min(), per[0].max(), np.array_equal(per[0], n_iter), gap_err, margin[0][0], margin[0][1])
        print(line)
    out["host_err"] = worst
    G.save("lassofit_" + name, **out)
    return worst_gap


def gen():
    worst = max(gen_case(name) for name in CASES)
    print("largest gap-form difference %.2e -> TIE = 100 x that" % worst)


if __name__ == "__main__":
    gen()
