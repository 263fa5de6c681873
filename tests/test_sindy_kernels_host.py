"""CPU preconditions of tests/test_gpu_sindy_kernels.py (no GPU): the libraries of tests/sindy_kernel_cases.py have
the sizes their tags promise, the host function that picks the MPPI rollout kernel (csrc/mppi_sindy_choice_host.hpp,
through the device-free ampc_mppi_sindy_launch_choice / ampc_sindy_pred_lds) sends every case to the intended body and
never asks for more than 160 KB of LDS, every feature of every library moves the oracle's result by far more than the
GPU test's tolerance, the oracle's rollouts are finite and its iLQR decisions robust."""
import numpy as np
import pytest

import sindy_kernel_cases as C
from autompc_amd import SINDy, _lib
from helpers import make_system, rel_err
from oracle.sindy import eval_features, feature_grads


@pytest.mark.parametrize("tag", sorted(C.CASES))
def test_sizes_staging_and_forward_lds_of_every_tag(tag):
    """n_feat / n_trig / n_tab, the f64 staging flag and sindy_forward_kernel's LDS bytes as the cases file lists them;
    the library's own answer (ampc_sindy_pred_lds) is the restated formula in both precisions."""
    c, sz = C.case(tag), C.sizes(tag)
    n_feat, n_trig, n_tab, staged, fwd = C.EXPECT[tag]
    assert (sz[1], sz[2], sz[6]) == (n_feat, n_trig, n_tab)
    assert (C.stage_bytes(sz, 8) > 0) == staged
    assert sz[6] == 2 * sz[2] + sz[3] + sz[4] + 1 or sz[6] == 0
    if fwd is not None:
        assert C.forward_lds(sz, c["nu"], 8) == fwd
    for precision, esz in (("f64", 8), ("f32", 4)):
        assert C.forward_lds(sz, c["nu"], esz) <= C.LDS_LIMIT                 # every tag's pred_batch is accepted
        assert _lib.sindy_pred_lds(sz, c["nu"], precision) == (C.stage_bytes(sz, esz) > 0, C.forward_lds(sz, c["nu"], esz))


def test_branch_markers_of_the_tags():
    """What the tags are FOR, from their sizes: which side of NR = 8, of kSindyMaxTab = 160, of the hoisted KF x G = 2 G
    features and of the first G trig arguments each one lies on."""
    sz = {t: C.sizes(t) for t in C.CASES}
    assert [sz[t][0] for t in C.SPREAD_TAGS] == [5, 8, 8, 6, 5, 7, 7, 8] and sz["s9"][0] == 9   # nx 5..8 spread, 9 beyond
    # feature counts on the hoisted 2 G themselves (32 / 64 / 128) and below the lanes of a group (12 < 16)
    assert [sz[t][1] for t in ("s5p", "s7", "s7t", "s8t")] == [12, 32, 64, 128] and sz["s5p"][2] == 0
    assert sz["s8t"][2] > 32                                                         # a third round of the trig loop at G = 16
    assert all(4 < sz[t][0] <= 8 and sz[t][6] > 0 and C.stage_bytes(sz[t], 8) > 0 for t in C.SPREAD_TAGS)
    assert sz["t160"][6] == 160 and sz["t163"][6] == 0                               # the table limit, both sides
    assert 2 * sz["t163"][2] == 0 and 2 * 54 + 54 + 1 == 163                         # (what t163's table would need)
    assert sz["s8"][2] > 16 and sz["s8w"][2] > 16 and sz["s5"][2] <= 16              # second trig loop at G = 16
    # features past the hoisted 2 G: s5 78 (> 32, > 64, <= 128), s8 60 (> 32, <= 64), s8w 70 (> 64), s6x 217 (> 128)
    assert 64 < sz["s5"][1] <= 128 and 32 < sz["s8"][1] <= 64 and 64 < sz["s8w"][1] <= 128 and sz["s6x"][1] > 128
    assert sz["s6x"][4] > 0 and sz["s6x"][3] > 0 and not C.case("s6x")["strict"]     # monomials and powers in the table
    assert (C.case("max")["nx"], C.case("max")["nu"]) == (64, 16)


def test_the_staging_pair_straddles_48_kb():
    lo, hi = C.staging_pair()
    assert hi == lo + 1
    below, above = C.prog_bytes(C.sizes("st_lo"), 8), C.prog_bytes(C.sizes("st_hi"), 8)
    assert below <= C.STAGE_LIMIT < above
    assert _lib.sindy_pred_lds(C.sizes("st_lo"), 1)[0] and not _lib.sindy_pred_lds(C.sizes("st_hi"), 1)[0]
    assert C.sizes("st_lo")[6] > 0 and C.sizes("st_hi")[6] > 0                       # both keep their product table


def _choice(tag, num_path, cap=C.HORIZON_CAP, precision="f64", **kw):
    c = C.case(tag)
    return _lib.sindy_launch_choice(C.sizes(tag), c["nu"], C.cost_stride(c["nx"], c["nu"]), cap, num_path, precision, **kw)


@pytest.mark.parametrize("precision,esz", [("f64", 8), ("f32", 4)])
def test_launch_choice_of_every_plan_the_gpu_test_builds(precision, esz):
    """Body, lanes and LDS bytes for every (tag, sample counts, AMPC_SINDY_G / AMPC_SINDY_FP) of the GPU test."""
    for problems in C.PLANS:
        N = [n for n, _ in problems]
        for tag in C.SPREAD_TAGS:
            c, sz = C.case(tag), C.sizes(tag)
            for G in (16, 32, 64):
                assert _choice(tag, N, precision=precision, g_forced=G) == dict(
                    spread=True, lanes=G, staged=True, lds_bytes=C.spread_lds(sz, c["nu"], esz, G, C.HORIZON_CAP))
            assert _choice(tag, N, precision=precision)["lanes"] == 64                # small plans: all 64 lanes
            assert _choice(tag, N, precision=precision, fp_allowed=False) == dict(
                spread=False, lanes=1, staged=True, lds_bytes=C.thread_lds(sz, c["nu"], esz))
        for tag in C.THREAD_TAGS:
            c, sz = C.case(tag), C.sizes(tag)
            for G in (0, 16):
                assert _choice(tag, N, precision=precision, g_forced=G) == dict(
                    spread=False, lanes=1, staged=C.stage_bytes(sz, esz) > 0, lds_bytes=C.thread_lds(sz, c["nu"], esz))
    assert _choice("s9", [5])["staged"] and not _choice("m40", [5])["staged"] and not _choice("m56", [5])["staged"]
    # the launcher's own choice of 32 and 16 lanes
    for n, h, lanes in C.NATURAL:
        assert C.natural_lanes([n]) == lanes
        assert _choice("s5", [n], cap=h, precision=precision) == _choice("s5", [n], cap=h, precision=precision, g_forced=lanes)
        assert _choice("s5", [n], cap=h, precision=precision)["lanes"] == lanes
    assert _choice("s5", [2048])["lanes"] == 64 and _choice("s5", [2049])["lanes"] == 32
    assert _choice("s5", [8192])["lanes"] == 32 and _choice("s5", [8193])["lanes"] == 16


def test_the_fall_back_when_the_lane_spread_map_does_not_fit():
    """lbf > kLdsLimit with nx <= 8.  The lane-spread map holds a noise row and a shifted action row of (horizon cap x
    nu) elements PER SAMPLE, the one-thread map none (it reads them from global memory), and the plan's own check counts
    one such row: a long horizon cap makes the lane-spread map the only one that does not fit.  Found by searching the
    cap on the host: s8w (8 / 6) at a cap of 1700 -- 2 x 10 200 doubles per sample at G = 64 -- where 1500 still fits."""
    tag, cap = C.FALLBACK
    c, sz = C.case(tag), C.sizes(tag)
    assert c["nx"] <= 8
    # the search: the first cap (in steps of 100) at which no lane grouping fits; the plan's own check -- the one-thread
    # columns, the cost block and ONE row of cap x nu -- still passes there
    first = next(k for k in range(100, 4000, 100) if min(C.spread_lds(sz, c["nu"], 8, G, k) for G in (16, 32, 64)) > C.LDS_LIMIT)
    assert first == cap and C.thread_lds(sz, c["nu"], 8) + cap * c["nu"] * 8 <= C.LDS_LIMIT
    for G in (16, 32, 64):
        assert C.spread_lds(sz, c["nu"], 8, G, cap) > C.LDS_LIMIT
    assert C.spread_lds(sz, c["nu"], 8, 64, 1500) <= C.LDS_LIMIT
    assert _choice(tag, [5], cap=1500) == dict(spread=True, lanes=64, staged=True,
                                               lds_bytes=C.spread_lds(sz, c["nu"], 8, 64, 1500))
    for G in (0, 16, 32, 64):
        assert _choice(tag, [5], cap=cap, g_forced=G) == dict(spread=False, lanes=1, staged=True,
                                                               lds_bytes=C.thread_lds(sz, c["nu"], 8))


def test_a_staged_program_that_does_not_fit_the_rollout_runs_unstaged_and_wide_plans_are_refused():
    """`lds`: sindy_forward_kernel fits with its staged program (161 216 B); the one-thread rollout with it would need
    177 072 B -- the launch used to ask for that after plan creation had passed a check without the program -- and is
    launched unstaged, at 129 008 B.  t160 / max: the columns and the cost block alone exceed 160 KB, a refusal."""
    c, sz = C.case("lds"), C.sizes("lds")
    assert C.prog_bytes(sz, 8) == 48048 and C.stage_bytes(sz, 8) == 48064
    assert C.thread_lds(sz, c["nu"], 8) == 177072 > C.LDS_LIMIT
    for problems in C.PLANS:
        got = _choice("lds", [n for n, _ in problems])
        assert got == dict(spread=False, lanes=1, staged=False, lds_bytes=C.thread_lds(sz, c["nu"], 8, staged=False))
        assert got["lds_bytes"] == 129008
    assert _choice("lds", [5], precision="f32")["staged"]                            # (f32: half the columns, it fits)
    for tag in C.MPPI_REFUSED:
        assert C.thread_lds(C.sizes(tag), C.case(tag)["nu"], 8, staged=False) > C.LDS_LIMIT
        with pytest.raises(_lib.AmpcError, match="do not fit the 160 KB LDS"):
            _choice(tag, [5])


def test_no_accepted_plan_or_prediction_asks_for_more_than_160_kb():
    """The sweep: nx 1..64, nu in (1, 6, 16), trig_freq 0..3, poly_degree 1..3, no interaction; both precisions; plans of
    5 / 2100 / 8200 samples at horizon caps 8 and 64, AMPC_SINDY_FP on and off, AMPC_SINDY_G unset / 16 / 64.  Every
    answer is either a refusal that names its reason or a request within 160 KB that the restated formulas reproduce."""
    seen = dict(pred_refused=0, plan_refused=0, unstaged_fallback=0, spread=0, thread=0)
    for nx in range(1, 65):
        for nu in (1, 6, 16):
            s = make_system(nx, nu)
            for trig in range(4):
                for poly in (1, 2, 3):
                    sz = C.sizes_of(SINDy(s, trig_basis=trig > 0, trig_freq=max(trig, 1), poly_basis=poly > 1, poly_degree=poly))
                    for precision, esz in (("f64", 8), ("f32", 4)):
                        want = C.forward_lds(sz, nu, esz)
                        try:
                            assert _lib.sindy_pred_lds(sz, nu, precision)[1] == want <= C.LDS_LIMIT
                        except _lib.AmpcError as e:
                            assert want > C.LDS_LIMIT and "staged" in str(e) and "160 KB" in str(e)
                            seen["pred_refused"] += 1
                        for n, cap, fp, G in ((5, 8, True, 0), (2100, 8, True, 0), (8200, 64, True, 0), (5, 64, False, 0),
                                              (130, 8, True, 16), (130, 64, True, 64)):
                            try:
                                got = _lib.sindy_launch_choice(sz, nu, C.cost_stride(nx, nu), cap, [n], precision, fp, G)
                            except _lib.AmpcError as e:
                                assert C.thread_lds(sz, nu, esz, staged=False) > C.LDS_LIMIT and "160 KB" in str(e)
                                seen["plan_refused"] += 1
                                continue
                            assert got["lds_bytes"] <= C.LDS_LIMIT
                            if got["spread"]:
                                assert fp and nx <= 8 and got["staged"] and got["lanes"] == (G or C.natural_lanes([n]))
                                assert got["lds_bytes"] == C.spread_lds(sz, nu, esz, got["lanes"], cap)
                                seen["spread"] += 1
                            else:
                                assert got["lanes"] == 1
                                assert got["lds_bytes"] == C.thread_lds(sz, nu, esz, staged=got["staged"])
                                if not got["staged"] and C.stage_bytes(sz, esz) > 0:
                                    assert C.thread_lds(sz, nu, esz) > C.LDS_LIMIT
                                    seen["unstaged_fallback"] += 1
                                seen["thread"] += 1
    print("sweep:", seen)
    # every kind of answer occurs in the sweep, but for a refused prediction: no library of this family has both a
    # table near 160 entries and a program small enough to be staged on 2 nx + nu columns (`lds`, 161 216 B, is as close
    # as they come).  The C ABI takes descriptor lists of any mix, so the guard is reachable: 79 sin features of 79
    # distinct arguments on 64 / 16 make a 159-entry table and a 42 KB staged program on 144 columns.
    assert all(v > 0 for k, v in seen.items() if k != "pred_refused") and seen["pred_refused"] == 0
    assert C.forward_lds(C.RAW_PRED_REFUSED, 16, 8) > C.LDS_LIMIT and C.stage_bytes(C.RAW_PRED_REFUSED, 8) > 0
    with pytest.raises(_lib.AmpcError, match="ampc_sindy_pred_batch.*staged feature program.*160 KB"):
        _lib.sindy_pred_lds(C.RAW_PRED_REFUSED, 16)
    assert _lib.sindy_pred_lds(C.RAW_PRED_REFUSED, 16, "f32")[1] == C.forward_lds(C.RAW_PRED_REFUSED, 16, 4)


@pytest.mark.parametrize("tag", C.ALL_TAGS)
def test_every_feature_counts(tag):
    """Zeroing column k of Xi changes the oracle's pred_batch on the test inputs by at least 1000 x the f64 tolerance
    of the GPU test (1e-12 relative, helpers.rel_err), and its Jacobian by 1000 x 1e-11 through at least one variable:
    a dropped, duplicated or mis-indexed feature cannot hide.  The model is linear in Xi, so the change is
    scale x outer(Theta[:, k], Xi[:, k]); three columns per tag are zeroed literally to check that identity.
    (The f32 runs at 1e-4 cannot see one coefficient of 0.01 .. 0.05 among 200; they check the f32 instantiations at
    f32's own precision, on tags whose every feature the f64 run has already pinned.)"""
    c = C.case(tag)
    orc, Xi = C.oracle(tag), np.array(C.coefficients(tag))
    s, u = C.inputs(tag)
    V = np.concatenate([s, u], axis=1)
    scale = C.DT if c["hyper"]["time_mode"] == "continuous" else 1.0
    pred, jx, ju = orc.pred_diff_batch(s, u)
    J = np.concatenate([jx, ju], axis=2)
    Theta = eval_features(orc.feats, V)
    G = feature_grads(orc.feats, V, orc.strict_reference)
    assert np.all(np.count_nonzero(Xi, axis=0) >= 1)
    mag = np.abs(Xi)
    assert np.max(mag, axis=0).min() >= 0.01 * 0.999                     # every column's largest entry
    d_pred = scale * np.max(np.abs(Theta), axis=0) * np.max(mag, axis=0) / np.max(np.abs(pred))
    d_jac = scale * np.max(np.abs(G), axis=(0, 2)) * np.max(mag, axis=0) / max(np.max(np.abs(jx)), np.max(np.abs(ju)))
    print("%s: smallest change by a feature: pred %.2e, Jacobian %.2e" % (tag, d_pred.min(), d_jac.min()))
    assert d_pred.min() >= 1000 * 1e-12 and d_jac.min() >= 1000 * 1e-11
    for k in (0, Xi.shape[1] // 2, Xi.shape[1] - 1):
        Z = Xi.copy()
        Z[:, k] = 0.0
        zp, zjx, zju = C.oracle(tag, Xi=Z).pred_diff_batch(s, u)
        assert abs(rel_err(zp, pred) / d_pred[k] - 1.0) < 1e-6
        assert max(np.max(np.abs(zjx - jx)), np.max(np.abs(zju - ju))) / np.max(np.abs(J)) >= 1000 * 1e-11


def test_s9_restricted_to_eight_states_is_an_eight_state_model():
    """Both sides of NR = 8 on one set of coefficients: a 9-state library whose first eight rows do not read the ninth
    state is, on those rows, the 8-state model built from the features that do not involve it."""
    Xi9, keep, Xi8 = C.s9_restriction()
    assert Xi8.shape[0] == 8 and Xi9.shape[0] == 9 and np.all(Xi9[:8, ~keep] == 0.0) and np.all(Xi9[8] != 0.0)
    s, u = C.inputs("s9")
    o9 = C.oracle("s9", Xi=Xi9).pred_batch(s, u)
    o8 = C.s9_oracle8().pred_batch(s[:, :8], u)
    assert rel_err(o9[:, :8], o8) < 1e-14
    assert np.all(np.count_nonzero(Xi8, axis=0) >= 1)


@pytest.mark.parametrize("cost", C.COSTS)
@pytest.mark.parametrize("tag", C.SPREAD_TAGS + C.THREAD_TAGS + ("lds",))
def test_every_rollout_of_the_cases_is_finite_on_the_cpu(tag, cost):
    clipped, levels = 0, set()
    for problems in C.PLANS:
        d = C.plan_data(tag, problems, cost)
        for b, (costs, eps, act) in enumerate(C.cpu_rollouts(tag, problems, cost)):
            assert costs.shape == (problems[b][0],) and np.all(np.isfinite(costs)) and np.all(np.abs(costs) < 1e6)
            assert np.all(np.isfinite(eps)) and np.all(np.isfinite(act))
            clipped += int(np.sum(eps != np.transpose(d["eps"][b], (1, 0, 2))))
        if cost == "dense":
            assert all(np.count_nonzero(d[k][0] - np.diag(np.diag(d[k][0]))) > 0 or d[k][0].shape[0] == 1 for k in "QRF")
            assert all(np.all(np.linalg.eigvalsh(d[k][0]) > 0) for k in "QRF")
    assert clipped > 0                                                   # the bounds bite somewhere


@pytest.mark.parametrize("tag", C.SPREAD_TAGS + C.THREAD_TAGS)
def test_indicator_terms_are_charged_on_some_rollouts_and_not_on_others(tag):
    quad = np.concatenate([r[0] for p in C.PLANS for r in C.cpu_rollouts(tag, p, "diag")])
    ind = np.concatenate([r[0] for p in C.PLANS for r in C.cpu_rollouts(tag, p, "indicator")])
    charge = np.round(ind - quad).astype(int)
    assert np.max(np.abs(ind - quad - charge)) < 1e-9 and charge.min() >= 0 and len(set(charge.tolist())) >= 2


def test_natural_lane_plans_are_finite_on_the_cpu():
    for n, h, _ in C.NATURAL:
        (costs, eps, act), = C.cpu_rollouts("s5", ((n, h),), "diag")
        assert costs.shape == (n,) and np.all(np.isfinite(costs)) and np.all(np.isfinite(act))


@pytest.mark.parametrize("H", C.ILQR_H)
@pytest.mark.parametrize("tag", C.ILQR_TAGS)
def test_the_oracles_ilqr_decisions_survive_a_perturbation_of_the_coefficients(tag, H):
    """1e-12 relative on Xi -- far more than the device's rounding differs from numpy's -- changes no decision and moves
    the trajectory by less than the GPU test's bound; the control bounds are active somewhere in the cases."""
    a, b = C.ilqr_oracle(tag, H), C.ilqr_oracle(tag, H, True)
    assert (a["converged"], a["iters"]) == (b["converged"], b["iters"])
    assert rel_err(b["states"], a["states"]) < 1e-8 and rel_err(b["ctrls"], a["ctrls"]) < 1e-8
    assert a["iters"] >= 1 and np.all(np.isfinite(a["states"]))
    assert np.all(a["ctrls"] >= C.ILQR_BOUNDS[0] - 1e-12) and np.all(a["ctrls"] <= C.ILQR_BOUNDS[1] + 1e-12)


def test_prototypes_of_the_new_entries():
    from ctypes import POINTER, c_int, c_longlong, c_void_p
    ip = POINTER(c_int)
    assert _lib.SIGNATURES["ampc_mppi_plan_sindy_launch"] == (c_int, [c_void_p, ip, ip, ip, ip])
    assert _lib.SIGNATURES["ampc_mppi_sindy_launch_choice"] == (c_int, [c_int] * 11 + [c_longlong, c_int, c_int, ip, ip, ip, ip])
    assert _lib.SIGNATURES["ampc_sindy_pred_lds"] == (c_int, [c_int] * 9 + [ip, ip])
    assert hasattr(_lib.MppiPlan, "sindy_launch")
