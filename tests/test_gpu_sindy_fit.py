"""Thresholded SINDy fits on the device (ampc_sindy_fit, sysid/sindy_fit.py) against the models' own train(), the
numpy form of the same algorithm, themselves in other batches, and through the evaluator.  Needs MI355X.

Tolerance (DESIGN 6d's rule): the device may be at most 100 x as far from train() as stlsq_gram_host is on that case,
floor 1e-13, both computed here on the host; the support must be equal.  No case held to that rule may decline: the
smallest threshold margin of the cases is 2.2e-5 (17 / 6, configuration 7; 8.0e-5 among the edge cases of
sindy_fit_cases.py), the smallest squared pivot 1.49e-7 n (272 features of the degree-6 library, 10 x the pivot line
2^-26 n = 1.49e-8 n); tests/test_sindy_fit_host.py asserts for every edge case that stlsq_gram_host alone fits it with
4 x the pivot line and 16 x the tie line to spare.  The cases that MUST decline (status 1, an all-NaN row) are the two
decline tests' own.
"""
import numpy as np
import pytest

from autompc_amd import ARXFactory, SINDy, SINDyFactory
from autompc_amd import _lib
from autompc_amd.evaluation import HoldoutModelEvaluator
from autompc_amd.sysid import sindy_fit as SF
from autompc_amd.tuning.configs import DictConfiguration
from linfit_cases import make_trajs, system
from sindy_fit_cases import (ALPHAS, BOTH, EDGE_KEPT, EDGE_SMALL, EDGE_WIDE, EDGES, ELIGIBLE, EXTREMES, LIMITS, LONG,
                             NEIGHBOURS, alpha_of, data, host_fit, new_model, rel_err, request, same_support, trained)

pytestmark = pytest.mark.gpu


def _fit(name, ks, xdot=False, **extra):
    args, kw = request(name, ks, xdot)
    return _lib.sindy_fit(*args, **dict(kw, **extra))


def _hold_to_train(name, k, out, slot=0, xdot=False):
    """The file's rule for configuration `slot` of a device result, every figure printed before it is asserted."""
    ref = trained(name, k, xdot)
    host = host_fit(name, k, xdot)
    coeffs, status, pivot, margin, iters = out
    tol = max(100.0 * rel_err(host[0], ref), 1e-13)
    err = rel_err(coeffs[slot], ref)
    print("sindy fit %s %s%s (%d features): device vs train() %.2e, stlsq_gram_host vs train() %.2e, device vs "
          "stlsq_gram_host %.2e, tolerance %.2e; pivot^2 %.2e, margin %.2e, %d solves"
          % (name, k, " xdot" if xdot else "", ref.shape[1], err, rel_err(host[0], ref),
             rel_err(coeffs[slot], host[0]), tol, pivot[slot], margin[slot], iters[slot]))
    assert status[slot] == 0
    assert same_support(coeffs[slot], ref) and err <= tol
    assert iters[slot] == host[4] and same_support(coeffs[slot], host[0])


def _same_bits(a, i, b, j):
    """Configuration i of result a is configuration j of result b: coefficients, status, pivot, margin, solves."""
    assert np.array_equal(a[0][i], b[0][j]) and np.all(np.isfinite(a[0][i]))
    assert all(a[q][i] == b[q][j] for q in (1, 2, 3, 4))


@pytest.mark.parametrize("name,k", ELIGIBLE)
def test_device_matches_train(name, k):
    ref = trained(name, k)
    host = host_fit(name, k)
    coeffs, status, pivot, margin, iters = _fit(name, [k])
    tol = max(100.0 * rel_err(host[0], ref), 1e-13)
    err = rel_err(coeffs[0], ref)
    print("sindy fit %s %d (%d features): device vs train() %.2e, stlsq_gram_host vs train() %.2e, device vs "
          "stlsq_gram_host %.2e, tolerance %.2e; pivot^2 %.2e, margin %.2e, %d solves"
          % (name, k, ref.shape[1], err, rel_err(host[0], ref), rel_err(coeffs[0], host[0]), tol, pivot[0], margin[0],
             iters[0]))
    assert status[0] == 0
    assert same_support(coeffs[0], ref) and err <= tol
    assert iters[0] == host[4] and same_support(coeffs[0], host[0])


@pytest.mark.parametrize("name,k", EDGE_SMALL + EDGE_WIDE + LIMITS + EDGE_KEPT)
def test_feature_counts_at_tile_edges_past_256_and_at_the_state_limit(name, k):
    """Alone in its call: 1, 15 .. 17, 31 .. 33 features (the 16-column tile), 255 .. 257 (the solve kernel's 256
    threads, fit_cholesky's rows = n + 1), 271 and 272 (the limit), 64 states with 16 controls, a second solve on one
    kept feature."""
    _hold_to_train(name, k, _fit(name, [k]))


@pytest.mark.parametrize("name,kd,kc", BOTH)
@pytest.mark.parametrize("xdot", [False, True])
def test_both_target_sets_in_one_design(name, kd, kc, xdot):
    """A discrete and a continuous configuration of one library make one design [Theta | Y_discrete | Y_continuous];
    alone, the continuous one's targets sit nx columns further left in a narrower design.  Same bits either way."""
    assert len(request(name, [kd, kc], xdot)[0][3]) == 1
    both, swapped = _fit(name, [kd, kc], xdot), _fit(name, [kc, kd], xdot)
    for i, k in enumerate((kd, kc)):
        _hold_to_train(name, k, both, i, xdot)
        _same_bits(both, i, _fit(name, [k], xdot), 0)
        _same_bits(both, i, swapped, 1 - i)
    assert not np.array_equal(both[0][0], both[0][1])


@pytest.mark.parametrize("order", [1, -1])
def test_designs_of_1_to_272_features_in_one_launch(order):
    name, ks = EXTREMES[0][0], [k for _, k in EXTREMES][::order]
    full = _fit(name, ks)
    assert len(request(name, ks)[0][3]) == len(ks) and np.all(full[1] == 0)
    for i, k in enumerate(ks):
        _same_bits(full, i, _fit(name, [k]), 0)


@pytest.mark.parametrize("name,k", ALPHAS)
def test_alpha_reaches_the_kernel(name, k):
    out = _fit(name, [k])
    assert alpha_of(k) != 0.05 and request(name, [k])[1]["alpha"] == alpha_of(k)
    _hold_to_train(name, k, out)
    assert not np.array_equal(out[0][0], _fit(name, [k[0]])[0][0])
    m = new_model(name, k)
    rep = SF.fit_sindy_models([m], data(name)[1], alpha=alpha_of(k))
    assert rep[0]["where"] == "device" and rep[0]["iters"] == host_fit(name, k)[4]
    assert np.array_equal(m.coefficients, out[0][0])


def _declines(out, lone, slot=1):
    """Configuration `slot` of a three-configuration call is declined by the pivot rule with an all-NaN row; its
    neighbours are bit for bit their lone calls (`lone`: one result per neighbour) and fitted."""
    assert list(out[1]) == [1 if i == slot else 0 for i in range(3)] and np.all(np.isnan(out[0][slot]))
    for i, alone in zip([i for i in range(3) if i != slot], lone):
        _same_bits(out, i, alone, 0)


def test_a_feature_twice_declines_by_the_pivot_rule_and_fits_with_the_ridge():
    n = new_model("small", "dup").library[0].shape[0]
    for a in (0.0, 1e-9):
        ks = [NEIGHBOURS[a][0][1], ("dup", a), NEIGHBOURS[a][1][1]]
        out = _fit("small", ks)
        print("sindy fit small dup alpha %g: status %s, pivot^2 %s, margin %s, solves %s"
              % (a, out[1], out[2], out[3], out[4]))
        _declines(out, [_fit("small", [ks[0]]), _fit("small", [ks[2]])])
        for _, k in NEIGHBOURS[a]:
            _hold_to_train("small", k, _fit("small", [k]))
    # (alpha 0: the failing pivot is pure cancellation, neither its value nor its sign is asserted)
    assert out[4][1] == 1 and 0.0 < out[2][1] < n * 2.0 ** -26               # alpha 1e-9: a finished solve
    _hold_to_train("small", "dup", _fit("small", ["dup"]))
    m = new_model("small", ("dup", 1e-9))
    rep = SF.fit_sindy_models([m], data("small")[1], alpha=1e-9)
    assert rep[0]["where"] == "host" and rep[0]["reason"] == "status 1" and rep.host_fits == 1
    assert rep[0]["iters"] == 1 and rep[0]["pivot"] == out[2][1]
    assert np.array_equal(m.coefficients, trained("small", ("dup", 1e-9)))


def test_a_zero_column_declines_at_the_diagonal():
    ks = [("states", 0.0), (1, 0.0), ("states_c", 0.0)]
    args, kw = request("small", ks)
    ctrls = np.zeros_like(args[2])
    out = _lib.sindy_fit(args[0], args[1], ctrls, args[3], args[4], **kw)
    print("sindy fit small zero control alpha 0: status %s, pivot^2 %s, solves %s" % (out[1], out[2], out[4]))
    lone = []
    for k in (ks[0], ks[2]):
        a, kw1 = request("small", [k])
        lone.append(_lib.sindy_fit(a[0], a[1], ctrls, a[3], a[4], **kw1))
        host = SF.stlsq_gram_host(a[0], a[1], ctrls, a[3], a[4], **kw1)
        assert host[1][0] == 0 and same_support(lone[-1][0][0], host[0][0]) and lone[-1][4][0] == host[4][0]
        assert rel_err(lone[-1][0][0], host[0][0]) <= 1e-9
    _declines(out, lone)
    assert out[2][1] == 0.0 and out[4][1] == 0


@pytest.mark.parametrize("name", ["small", "hc"])
def test_a_configuration_has_the_same_bits_in_any_batch(name):
    ks = [k for n, k in ELIGIBLE if n == name]
    full = _fit(name, ks)
    again = _fit(name, ks)
    perm = ks[::-1][2:] + ks[::-1][:2]
    permuted = _fit(name, perm)
    assert np.all(full[1] == 0)
    for i, k in enumerate(ks):
        alone = _fit(name, [k])
        j = perm.index(k)
        for other, slot in ((again, i), (permuted, j), (alone, 0)):
            assert np.array_equal(full[0][i], other[0][slot])
            assert full[2][i] == other[2][slot] and full[3][i] == other[3][slot] and full[4][i] == other[4][slot]


@pytest.mark.parametrize("name,k", LONG)
def test_three_row_splits(name, k):
    ref = trained(name, k)
    coeffs, status, pivot, margin, iters = _fit(name, [k])
    host = host_fit(name, k)
    assert status[0] == 0 and same_support(coeffs[0], ref)
    assert rel_err(coeffs[0], ref) <= max(100.0 * rel_err(host[0], ref), 1e-13)


def test_row_edges_and_rows_that_must_not_be_formed():
    """"edges": a trajectory ends on the last row of a split, a whole split has no design row, the last 16-row chunk
    holds one row and that row has no successor.  NaN in the 513 one-row trajectories changes no bit: such a row has no
    successor and is nobody's next observation, so it is dropped by a select and none of its values is formed."""
    name, ks = EDGES[0][0], [k for _, k in EDGES]
    args, kw = request(name, ks)
    lens = np.asarray(args[0])
    assert len(args[1]) == 1057 and np.cumsum(lens)[0] == 512 and np.all(lens[1:513] == 1) and lens[-1] == 1
    out = _lib.sindy_fit(*args, **kw)
    for i, k in enumerate(ks):
        _hold_to_train(name, k, out, i)
    rows = (np.cumsum(lens) - 1)[lens == 1]
    obs, ctrls = args[1].copy(), args[2].copy()
    obs[rows], ctrls[rows] = np.nan, np.nan
    assert len(rows) == 513 and rows[-1] == 1056
    poisoned = _lib.sindy_fit(args[0], obs, ctrls, args[3], args[4], **kw)
    for i in range(len(ks)):
        _same_bits(out, i, poisoned, i)


def test_near_tie_and_max_iter_on_the_device():
    (lens, obs, ctrls, designs, _), _ = request("small", [3])
    first = _lib.sindy_fit(lens, obs, ctrls, designs, [(0, False, 0.0)], max_iter=1)
    assert first[1][0] == 0 and first[4][0] == 1 and np.isinf(first[3][0])
    w = np.sort(np.abs(first[0][0][0]))[len(first[0][0][0]) // 2]
    thr = float(w * (1.0 + 2.0 ** -24))
    _, status, _, margin, _ = _lib.sindy_fit(lens, obs, ctrls, designs, [(0, False, thr), (0, False, 0.02)])
    assert list(status) == [2, 0] and margin[0] < SF.TIE_MARGIN
    m = new_model("small", 3, threshold=thr)
    rep = SF.fit_sindy_models([m], data("small")[1])
    ref = new_model("small", 3, threshold=thr)
    ref.train(data("small")[1])
    assert rep[0]["reason"] == "status 2" and rep.host_fits == 1 and np.array_equal(m.coefficients, ref.coefficients)
    # max_iter ends the loop right after a drop (natural count 7)
    m2, ref2 = new_model("hc", 3), new_model("hc", 3)
    rep = SF.fit_sindy_models([m2], data("hc")[1], max_iter=2)
    ref2.train(data("hc")[1], max_iter=2)
    assert rep[0]["where"] == "device" and rep[0]["iters"] == 2 and same_support(m2.coefficients, ref2.coefficients)
    assert rel_err(m2.coefficients, ref2.coefficients) <= 1e-9


def test_refusals():
    (lens, obs, ctrls, designs, configs), kw = request("small", [3])
    with pytest.raises(_lib.AmpcError, match="max_iter < 1"):
        _lib.sindy_fit(lens, obs, ctrls, designs, configs, max_iter=0)
    with pytest.raises(_lib.AmpcError, match="needs continuous targets"):
        _lib.sindy_fit(lens, obs, ctrls, designs, [(0, True, 0.1)])
    s17 = system(17, 6)
    big = SINDy(s17, poly_basis=True, poly_degree=8, trig_basis=True, trig_freq=3)
    a, _ = request("hc", [1])
    with pytest.raises(_lib.AmpcError, match="1..272 features"):
        _lib.sindy_fit(a[0], a[1], a[2], [big.library], [(0, False, 0.01)])
    wide = np.zeros((len(obs), 65))
    with pytest.raises(_lib.AmpcError, match="obs_dim must be in 1..64"):
        _lib.sindy_fit(lens, wide, ctrls, designs, configs)
    bad = tuple(np.array(x) for x in designs[0])
    bad[1][0] = 4                                               # a variable past [obs | ctrls]
    with pytest.raises(_lib.AmpcError, match="variable out of range"):
        _lib.sindy_fit(lens, obs, ctrls, [bad], configs)


class _MixedFactory:
    """SINDy configurations and, for ``family == "arx"``, an ARX model: one ``evaluate_batch`` with both."""
    name = "mixed"

    def __init__(self, s):
        self.sindy, self.arx = SINDyFactory(s), ARXFactory(s)

    def __call__(self, cfg, train_trajs, silent=False, skip_train_model=False):
        d = dict(cfg.get_dictionary())
        family = d.pop("family")
        return (self.arx if family == "arx" else self.sindy)(DictConfiguration(d), train_trajs, silent=silent,
                                                              skip_train_model=skip_train_model)


def test_holdout_evaluator_fits_a_batch_in_one_call_and_agrees_with_the_host_fit(monkeypatch):
    s = system(3, 1)
    trajs = make_trajs(s, [60] * 12, 11)
    trig = dict(family="sindy", trig_basis="true", trig_freq=1)
    poly = dict(family="sindy", poly_basis="true", poly_degree=3)
    kws = [dict(trig, threshold=0.02, time_mode="discrete"), dict(poly, threshold=0.01, time_mode="discrete"),
           dict(family="arx", history=2),
           dict(trig, threshold=0.05, time_mode="continuous"), dict(poly, threshold=0.03, time_mode="discrete")]
    cfgs = [DictConfiguration(kw) for kw in kws]
    horizon = 5
    kw = dict(horizon=horizon, holdout_prop=0.25, sindy_kstep="device")
    host = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), **kw)
    dev = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), sindy_fit="device", **kw)
    calls = []
    real = _lib.sindy_fit
    monkeypatch.setattr(_lib, "sindy_fit", lambda *a, **k: calls.append(len(a[4])) or real(*a, **k))
    a = np.asarray(host.evaluate_batch(_MixedFactory(s), cfgs))
    assert calls == [] and host.last_sindy_fit is None
    b = np.asarray(dev.evaluate_batch(_MixedFactory(s), cfgs))
    rep = dev.last_sindy_fit
    assert calls == [4] and len(rep) == 4 and rep.host_fits == 0 and rep.device_fits == 4 and rep.designs == 2
    assert all(r["where"] == "device" for r in rep)
    # coefficient tolerance of the batch: the rule above on the training set, the largest of its four configurations
    ctol = 0.0
    for kw_ in kws:
        if kw_["family"] != "sindy":
            continue
        d = {k: v for k, v in kw_.items() if k != "family"}
        m, ref = SINDyFactory(s)(DictConfiguration(d), dev.training_set, skip_train_model=True), None
        ref = SINDyFactory(s)(DictConfiguration(d), dev.training_set)
        SF.fit_sindy_models([m], dev.training_set, backend="numpy")
        ctol = max(ctol, 100.0 * rel_err(m.coefficients, ref.coefficients), 1e-13)
    tol = 10 * ctol * horizon
    diff = np.abs(a - b) / np.abs(a)
    print("evaluator: scores %s; max relative score difference %.2e (tolerance %.2e)"
          % (np.array2string(b, precision=4), diff.max(), tol))
    assert np.all(np.isfinite(a)) and diff.max() <= tol
    assert a[2] == b[2]                                         # the ARX model is fitted and scored as before
