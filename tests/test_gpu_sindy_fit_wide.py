"""Thresholded SINDy fits of libraries of up to 2048 features on the device (ampc_sindy_fit_wide, sysid/sindy_fit.py)
against the models' own train(), the numpy form of the same algorithm, themselves in other batches and under another
wave cut, and through the evaluator.  Needs MI355X.

Tolerance (DESIGN 6d's rule, as tests/test_gpu_sindy_fit.py): the device may be at most 100 x as far from train() as
stlsq_gram_host is on that case, floor 1e-13, both computed here on the host; the support and the solve count must be
equal.  tests/test_sindy_fit_wide_host.py asserts for every such case that stlsq_gram_host alone fits it with 4 x the
pivot line and 16 x the tie line to spare.  The cases that MUST decline are the decline tests' own.
"""
import numpy as np
import pytest

from autompc_amd import ARXFactory, SINDyFactory
from autompc_amd import _lib
from autompc_amd.evaluation import HoldoutModelEvaluator
from autompc_amd.sysid import sindy_fit as SF
from autompc_amd.sysid.sindy import build_library
from autompc_amd.trajectory import Trajectory
from autompc_amd.tuning.configs import DictConfiguration
from linfit_cases import make_trajs, system
from sindy_fit_wide_cases import (EDGE_ROWS, MIXED, PANEL, SHRINK, SIZES, THRESHOLD, data, first_features, host_fit,
                                  library, new_model, only_states, rel_err, request, same_support, support_of, trained,
                                  with_duplicate, xdot)

pytestmark = pytest.mark.gpu


def _fit(name, n, kept=None, **extra):
    args, kw = request(name, n, kept)
    return _lib.sindy_fit_wide(*args, **dict(kw, **extra))


def _hold_to_train(name, n, out, slot=0, kept=None):
    """The file's rule for configuration `slot` of a device result, every figure printed before it is asserted."""
    ref, host = trained(name, n, kept), host_fit(name, n, kept)
    coeffs, status, pivot, margin, iters = out
    tol = max(100.0 * rel_err(host[0], ref), 1e-13)
    err = rel_err(coeffs[slot], ref)
    print("wide sindy fit %s %d kept %s: device vs train() %.2e, stlsq_gram_host vs train() %.2e, device vs "
          "stlsq_gram_host %.2e, tolerance %.2e; pivot^2 %.3e (host %.3e), margin %.3e, %d solves, status %d"
          % (name, n, kept, err, rel_err(host[0], ref), rel_err(coeffs[slot], host[0]), tol, pivot[slot], host[2],
             margin[slot], iters[slot], status[slot]))
    assert status[slot] == 0
    assert same_support(coeffs[slot], ref) and err <= tol
    assert iters[slot] == host[4] and same_support(coeffs[slot], host[0])


def _same_bits(a, i, b, j):
    """Configuration i of result a is configuration j of result b: coefficients, status, pivot, margin, solves."""
    assert np.array_equal(a[0][i], b[0][j]) and np.all(np.isfinite(a[0][i]))
    assert all(a[q][i] == b[q][j] for q in (1, 2, 3, 4))


@pytest.mark.parametrize("name,n", SIZES)
def test_feature_counts_alone_in_their_call(name, n):
    """1, 17 and 272 (the narrow path's sizes through the wide entry), 273, around 288 (panel width 32), 384 (a wave's
    run of 8 tiles in the Gram pass) and 512 (the column block of the kernel that materialises Theta), 2047, 2048."""
    _hold_to_train(name, n, _fit(name, n))


def test_refusals():
    (lens, obs, ctrls, designs, configs), kw = request("big", 2048)
    with pytest.raises(_lib.AmpcError, match="ampc_sindy_fit_wide: a design must have 1..2048 features"):
        _lib.sindy_fit_wide(lens, obs, ctrls, [library("big", 2049)], configs, **kw)
    with pytest.raises(_lib.AmpcError, match="ampc_sindy_fit_wide: obs_dim must be in 1..64"):
        _lib.sindy_fit_wide(lens, np.zeros((len(obs), 65)), ctrls, designs, [(0, False, 0.1)])
    with pytest.raises(_lib.AmpcError, match="ampc_sindy_fit_wide: ctrl_dim must be in 1..16"):
        _lib.sindy_fit_wide(lens, obs, np.zeros((len(obs), 17)), designs, [(0, False, 0.1)])
    bad = tuple(np.array(x) for x in designs[0])
    bad[1][0] = 2                                               # a variable past [obs | ctrls]
    with pytest.raises(_lib.AmpcError, match="ampc_sindy_fit_wide: feature variable out of range"):
        _lib.sindy_fit_wide(lens, obs, ctrls, [bad], configs, **kw)
    (lens, obs, ctrls, designs, configs), kw = request("s", 273)
    with pytest.raises(_lib.AmpcError, match="ampc_sindy_fit: a design must have 1..272 features"):
        _lib.sindy_fit(lens, obs, ctrls, designs, configs, **kw)


@pytest.mark.parametrize("name,n,kept", SHRINK)
def test_second_solve_on_one_feature_and_just_past_a_panel_edge(name, n, kept):
    """n changes between the solves (300 -> 1, 300 -> 33), rows = n + 1, back substitution at the new size."""
    out = _fit(name, n, kept)
    _hold_to_train(name, n, out, kept=kept)
    assert out[4][0] == 2 and np.count_nonzero(out[0][0][0]) == kept and kept in (1, PANEL + 1)
    assert np.array_equal(np.nonzero(out[0][0][0])[0], support_of(n, kept))


def test_both_target_sets_in_one_design():
    """A discrete (threshold 0: its targets are noise, one solve) and a continuous configuration of one wide library
    make one design [Theta | Y_discrete | Y_continuous].  Same bits as alone and as in the swapped call."""
    (lens, obs, ctrls, designs, cc), kw = request("s", 400)
    cd = [(0, False, 0.0)]
    both = _lib.sindy_fit_wide(lens, obs, ctrls, designs, cd + cc, **kw)
    swapped = _lib.sindy_fit_wide(lens, obs, ctrls, designs, cc + cd, **kw)
    _hold_to_train("s", 400, both, 1)
    m = new_model("s", designs[0], threshold=0.0, time_mode="discrete")
    m.train(data("s")[1])
    host = SF.stlsq_gram_host(lens, obs, ctrls, designs, cd)
    tol = max(100.0 * rel_err(host[0][0], m.coefficients), 1e-13)
    err = rel_err(both[0][0], m.coefficients)
    print("wide sindy fit s 400 discrete: device vs train() %.2e, host vs train() %.2e, tolerance %.2e, %d solves"
          % (err, rel_err(host[0][0], m.coefficients), tol, both[4][0]))
    assert both[1][0] == 0 and both[4][0] == 1 == host[4][0] and err <= tol and np.isinf(both[3][0])
    for i, c in enumerate((cd, cc)):
        _same_bits(both, i, _lib.sindy_fit_wide(lens, obs, ctrls, designs, c, **(kw if c is cc else {})), 0)
        _same_bits(both, i, swapped, 1 - i)
    assert not np.array_equal(both[0][0], both[0][1])


def _mixed_request(cases, name="s"):
    """One call with a design per (name, n) case: each on its own xdot is not possible in one call, so all share the
    first case's targets (the support then differs from the cases' own: only bits are compared)."""
    (lens, obs, ctrls, _, _), kw = request(*cases[0])
    return (lens, obs, ctrls, [library(nm, n) for nm, n in cases], [(i, True, THRESHOLD) for i in range(len(cases))]), kw


@pytest.mark.parametrize("order", [1, -1])
def test_designs_of_different_widths_in_one_launch(order):
    """273, 400 and 513 features in one launch, forwards and reversed, and 17 and 2048 in one launch on the big data
    set: each the same bits as alone and from run to run."""
    for cases in (MIXED[::order], [("big", 17), ("big", 2048)][::order]):
        args, kw = _mixed_request(cases, cases[0][0])
        full, again = _lib.sindy_fit_wide(*args, **kw), _lib.sindy_fit_wide(*args, **kw)
        assert np.all(full[1] == 0)
        for i in range(len(cases)):
            alone = _lib.sindy_fit_wide(args[0], args[1], args[2], [args[3][i]], [(0, True, THRESHOLD)], **kw)
            _same_bits(full, i, alone, 0)
            _same_bits(full, i, again, i)
        if cases[0] == ("s", 273):
            _hold_to_train("s", 273, full)             # (slot 0 on its own targets: the rule)


def _model_ends_as_train(lib, trajs, xd, alpha, reason, threshold=THRESHOLD):
    m, ref = new_model("s", lib, threshold), new_model("s", lib, threshold)
    rep = SF.fit_sindy_models([m], trajs, xdot=xd, alpha=alpha, wide="device")
    ref.train(trajs, xdot=xd, alpha=alpha)
    assert rep[0]["where"] == "host" and rep[0]["reason"] == reason and rep[0]["route"] == "wide"
    assert rep.host_fits == 1 and rep.device_fits == 0 and np.array_equal(m.coefficients, ref.coefficients)
    return rep


def test_a_feature_twice_declines_by_the_pivot_rule():
    """A 301-feature library with feature 40 twice between two good neighbours, at alpha 1e-9 (the ridge term that
    makes the solve finish: the pivot is then about 1e-12, below the line)."""
    (lens, obs, ctrls, _, _), kw = request("s", 300)
    dup = with_duplicate(library("s", 300), 40)
    designs = [library("s", 273), dup, library("s", 400)]
    cfgs = [(i, True, THRESHOLD) for i in range(3)]
    out = _lib.sindy_fit_wide(lens, obs, ctrls, designs, cfgs, alpha=1e-9, **kw)
    print("wide sindy fit dup: status %s, pivot^2 %s, margin %s, solves %s" % (out[1], out[2], out[3], out[4]))
    assert list(out[1]) == [0, 1, 0] and np.all(np.isnan(out[0][1]))
    assert out[4][1] == 1 and 0.0 < out[2][1] < 301 * 2.0 ** -26
    for i in (0, 2):
        _same_bits(out, i, _lib.sindy_fit_wide(lens, obs, ctrls, [designs[i]], cfgs[:1], alpha=1e-9, **kw), 0)
    rep = _model_ends_as_train(dup, data("s")[1], xdot("s", 300), 1e-9, "status 1")
    assert rep[0]["pivot"] == out[2][1] and rep[0]["iters"] == 1


def test_a_zero_column_declines_at_the_diagonal():
    """Zero controls at alpha 0: the control's own column is zero and the design that holds it is declined before any
    solve; its neighbours read the states only.  train() itself raises for that design (a singular matrix), and so does
    fit_sindy_models, which hands it to train()."""
    s, trajs = data("s")
    (lens, obs, ctrls, _, _), kw = request("s", 300)
    ctrls = np.zeros_like(ctrls)
    states = only_states(build_library(3, trig_freq=60, trig_interaction=True), 2)
    designs = [first_features(states, 273), library("s", 300), first_features(states, 300)]
    cfgs = [(i, True, THRESHOLD) for i in range(3)]
    out = _lib.sindy_fit_wide(lens, obs, ctrls, designs, cfgs, alpha=0.0, **kw)
    print("wide sindy fit zero control alpha 0: status %s, pivot^2 %s, solves %s" % (out[1], out[2], out[4]))
    assert list(out[1]) == [0, 1, 0] and np.all(np.isnan(out[0][1])) and out[2][1] == 0.0 and out[4][1] == 0
    for i in (0, 2):
        lone = _lib.sindy_fit_wide(lens, obs, ctrls, [designs[i]], cfgs[:1], alpha=0.0, **kw)
        _same_bits(out, i, lone, 0)
        host = SF.stlsq_gram_host(lens, obs, ctrls, [designs[i]], cfgs[:1], alpha=0.0, **kw)
        assert host[1][0] == 0 and same_support(lone[0][0], host[0][0]) and lone[4][0] == host[4][0]
        assert rel_err(lone[0][0], host[0][0]) <= 1e-9
    zero = [Trajectory(s, len(t), t.obs, np.zeros_like(t.ctrls)) for t in trajs]
    for fit in (lambda m: m.train(zero, xdot=xdot("s", 300), alpha=0.0),
                lambda m: SF.fit_sindy_models([m], zero, xdot=xdot("s", 300), alpha=0.0, wide="device")):
        with pytest.raises(np.linalg.LinAlgError):
            fit(new_model("s", library("s", 300)))


def test_a_near_tie_declines_by_the_tie_rule():
    (lens, obs, ctrls, designs, _), kw = request("s", 300)
    first = _lib.sindy_fit_wide(lens, obs, ctrls, designs, [(0, True, 0.0)], max_iter=1, **kw)
    assert first[1][0] == 0 and first[4][0] == 1 and np.isinf(first[3][0])
    w = np.sort(np.abs(first[0][0][0]))[150]
    thr = float(w * (1.0 + 2.0 ** -24))
    out = _lib.sindy_fit_wide(lens, obs, ctrls, designs, [(0, True, thr), (0, True, THRESHOLD)], **kw)
    print("wide sindy fit tie: status %s, margin %s, solves %s" % (out[1], out[3], out[4]))
    assert list(out[1]) == [2, 0] and out[3][0] < SF.TIE_MARGIN
    _same_bits(out, 1, _fit("s", 300), 0)
    _model_ends_as_train(designs[0], data("s")[1], xdot("s", 300), 0.05, "status 2", threshold=thr)


def test_row_edges_and_rows_that_must_not_be_formed():
    """"edges": a trajectory ends on the last row of a split, a whole split has no design row, the last chunk holds one
    row and that row has no successor.  NaN in the 513 one-row trajectories (observations, controls and targets)
    changes no bit: such a row is dropped by a select and none of its values is formed."""
    for name, n in EDGE_ROWS:
        args, kw = request(name, n)
        lens = np.asarray(args[0])
        assert len(args[1]) == 1057 and np.cumsum(lens)[0] == 512 and np.all(lens[1:513] == 1) and lens[-1] == 1
        out = _lib.sindy_fit_wide(*args, **kw)
        _hold_to_train(name, n, out)
        rows = (np.cumsum(lens) - 1)[lens == 1]
        obs, ctrls, ycont = args[1].copy(), args[2].copy(), kw["ycont"].copy()
        obs[rows], ctrls[rows], ycont[rows] = np.nan, np.nan, np.nan
        assert len(rows) == 513 and rows[-1] == 1056
        _same_bits(out, 0, _lib.sindy_fit_wide(args[0], obs, ctrls, args[3], args[4], ycont=ycont), 0)


def test_the_wave_cut_changes_no_bit(monkeypatch):
    """A budget of 6 MiB, of which the three Grams take 4.3 MB: every design's four row splits (1.2 .. 2.2 MB of
    materialised rows each) go through the Gram pass one wave at a time, the 513-feature design's two pairs (2.1 MB of
    workspace each) through the solve one wave at a time."""
    args, kw = _mixed_request(MIXED)
    full = _lib.sindy_fit_wide(*args, **kw)
    monkeypatch.setenv("AMPC_SINDY_WIDE_BUDGET_MB", "6")
    cut = _lib.sindy_fit_wide(*args, **kw)
    for i in range(len(MIXED)):
        _same_bits(full, i, cut, i)
    _hold_to_train("s", 273, cut)


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


def test_holdout_evaluator_makes_one_call_of_each_entry(monkeypatch):
    """A narrow (12 features), a wide (4 + 32 * 9 = 292 features; on the host: six solves, smallest squared pivot
    9.6e-4 = 220 x the line, margin 0.011) and an ARX configuration in one batch."""
    s = system(3, 1)
    trajs = make_trajs(s, [100] * 12, 11)
    kws = [dict(family="sindy", trig_basis="true", trig_freq=1, threshold=0.02, time_mode="discrete"),
           dict(family="sindy", trig_basis="true", trig_freq=9, trig_interaction="true", threshold=0.02,
                time_mode="discrete"),
           dict(family="arx", history=2)]
    cfgs = [DictConfiguration(kw) for kw in kws]
    horizon = 5
    kw = dict(horizon=horizon, holdout_prop=0.25, sindy_kstep="device")
    host = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), **kw)
    dev = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), sindy_fit="device",
                                sindy_wide_fit="device", **kw)
    calls = []
    for entry in ("sindy_fit", "sindy_fit_wide"):
        real = getattr(_lib, entry)
        monkeypatch.setattr(_lib, entry, lambda *a, _e=entry, _r=real, **k: calls.append((_e, len(a[4]))) or _r(*a, **k))
    a = np.asarray(host.evaluate_batch(_MixedFactory(s), cfgs))
    assert calls == [] and host.last_sindy_fit is None
    b = np.asarray(dev.evaluate_batch(_MixedFactory(s), cfgs))
    rep = dev.last_sindy_fit
    print("evaluator: calls %s, report %s" % (calls, list(rep)))
    assert calls == [("sindy_fit", 1), ("sindy_fit_wide", 1)]
    assert len(rep) == 2 and rep.host_fits == 0 and rep.device_fits == 2 and rep.designs == 2
    assert [r["route"] for r in rep] == ["narrow", "wide"] and all(r["where"] == "device" for r in rep)
    ctol = 0.0
    for kw_ in kws[:2]:
        d = {k: v for k, v in kw_.items() if k != "family"}
        m = SINDyFactory(s)(DictConfiguration(d), dev.training_set, skip_train_model=True)
        ref = SINDyFactory(s)(DictConfiguration(d), dev.training_set)
        SF.fit_sindy_models([m], dev.training_set, backend="numpy", wide="device")
        ctol = max(ctol, 100.0 * rel_err(m.coefficients, ref.coefficients), 1e-13)
    tol = 10 * ctol * horizon
    diff = np.abs(a - b) / np.abs(a)
    print("evaluator: scores %s / %s; max relative score difference %.2e (tolerance %.2e)"
          % (np.array2string(a, precision=4), np.array2string(b, precision=4), diff.max(), tol))
    assert np.all(np.isfinite(a)) and diff.max() <= tol
    assert a[2] == b[2]                                         # the ARX model is fitted and scored as before
