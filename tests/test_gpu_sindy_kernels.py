"""The single-model SINDy kernels (csrc/sindy_kernels.hpp: sindy_forward_kernel, sindy_jacobian_kernel,
mppi_rollout_sindy_kernel, mppi_rollout_sindy_fp_kernel) past CartPole's four states, across the table and staging
limits and every lane grouping, against the numpy oracle (oracle/sindy.py, oracle/mppi.py, oracle/ilqr.py).
Libraries, coefficients, inputs and plans: tests/sindy_kernel_cases.py; their CPU preconditions (sizes, the launcher's
choice, "every feature counts", finite rollouts): tests/test_sindy_kernels_host.py.  Needs MI355X.

Bounds are tests/test_gpu_sindy.py's: predictions 1e-12 and Jacobians 1e-11 (f64), 1e-4 and 1e-3 (f32), MPPI costs 1e-10
and updated sequence 1e-9, all with helpers.rel_err."""
import functools

import numpy as np
import pytest

import sindy_kernel_cases as C
from helpers import rel_err

pytestmark = pytest.mark.gpu

# libraries with interaction or power terms run with strict_reference both ways (s8w has neither: it does not enter)
BOTH_WAYS = tuple(t for t in C.ALL_TAGS if t != "s8w")


# ---- model surface ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_surface(tag, strict):
    s, u = C.inputs(tag)
    return C.oracle(tag, strict).pred_diff_batch(s, u)


def _surface(m, ref, s, u, tol_p, tol_j, what):
    eo, ejx, eju = ref
    worst = [0.0, 0.0]
    for n in C.ROWS:
        errs = [rel_err(m.pred_batch(s[:n], u[:n]), eo[:n])]
        o, jx, ju = m.pred_diff_batch(s[:n], u[:n])
        errs += [rel_err(o, eo[:n]), rel_err(jx, ejx[:n]), rel_err(ju, eju[:n])]
        print("%s, %d rows: pred %.2e / %.2e  Jx %.2e  Ju %.2e" % ((what, n) + tuple(errs)))
        worst = [max(worst[0], errs[0], errs[1]), max(worst[1], errs[2], errs[3])]
        assert errs[0] < tol_p and errs[1] < tol_p and errs[2] < tol_j and errs[3] < tol_j, (what, n)
    assert rel_err(m.pred(s[7], u[7]), eo[7]) < tol_p
    o, jx, ju = m.pred_diff(s[129], u[129])
    assert rel_err(o, eo[129]) < tol_p and rel_err(jx, ejx[129]) < tol_j and rel_err(ju, eju[129]) < tol_j
    return worst


@pytest.mark.parametrize("tag,strict", [(t, True) for t in C.ALL_TAGS] + [(t, False) for t in BOTH_WAYS])
def test_pred_and_jacobian_match_the_oracle_f64(tag, strict):
    """sindy_step through pred_batch and sindy_jacobian_kernel through pred_diff_batch on 1, 63, 64, 65 and 130 rows:
      s5 .. s8w, s6x  register accumulation (nx <= NR = 8) at 5, 6 and 8 states; s6x: powers and monomials in the table,
                      the Jacobian's monomial, power and interaction branches strict and not
      s9, lds, st_lo  LDS read-modify-write accumulation (nx > 8) on a staged program
      t160            n_tab = 160, the largest product table, unstaged; m40 the same at 139
      t163            n_tab would be 163: direct evaluation (n_tab == 0) through pred_batch and the Jacobian
      max, m56        64 / 16 and 56 / 16: a 64 x 64 Jx and 64 x 16 Ju per thread, a power-only table
      st_lo / st_hi   the staging pair: a 45 656-byte program staged, a 56 000-byte one read from global memory
      lds             the forward kernel at 161 216 B of LDS, just inside the limit
    Measured on MI355X: predictions <= 6.7e-16, Jacobians <= 3.7e-16 over all tags and row counts -- every tag meets the
    CartPole bounds as they stand; none needed a bound from an extended-precision measurement of the oracle."""
    s, u = C.inputs(tag)
    _surface(C.model(tag, "f64", strict), _oracle_surface(tag, strict), s, u, 1e-12, 1e-11, "%s f64 strict=%s" % (tag, strict))


@pytest.mark.parametrize("tag", C.F32_TAGS)
def test_pred_and_jacobian_match_the_oracle_f32(tag):
    """The f32 instantiations: a staged program of floats with the int arrays behind it at 4-byte granularity (s5, s8,
    s9), t160's table staged in f32 (42 416 B) where f64 does not stage it, direct evaluation (t163).
    Measured on MI355X: predictions <= 3.2e-7, Jacobians <= 1.4e-7."""
    s, u = C.inputs(tag)
    strict = C.case(tag)["strict"]
    _surface(C.model(tag, "f32", strict), _oracle_surface(tag, strict), s, u, 1e-4, 1e-3, "%s f32" % tag)


def test_s9_restricted_to_eight_states_is_the_eight_state_model():
    """Both sides of NR = 8 on one construction (sindy_kernel_cases.s9_restriction): the 9-state model's first eight
    rows (LDS accumulation) and the 8-state model (register accumulation) both match the oracle of the 8-state model."""
    Xi9, _, _ = C.s9_restriction()
    s, u = C.inputs("s9")
    want = C.s9_oracle8().pred_batch(s[:, :8], u)
    got9 = C.model("s9", Xi=Xi9).pred_batch(s, u)
    got8 = C.s9_model8().pred_batch(s[:, :8], u)
    print("s9 restricted: nine-state rows %.2e, eight-state model %.2e" % (rel_err(got9[:, :8], want), rel_err(got8, want)))
    assert rel_err(got9[:, :8], want) < 1e-12 and rel_err(got8, want) < 1e-12
    assert rel_err(got9, C.oracle("s9", Xi=Xi9).pred_batch(s, u)) < 1e-12


# ---- single-model MPPI rollouts --------------------------------------------------------------------------------------
def _solve(tag, problems, cost="diag", precision="f64", cap=C.HORIZON_CAP, expect=None):
    """One solve of a plan over `problems` on the tag's model with the case's noise.  expect: what
    MppiPlan.sindy_launch() must report before the solve (keys of its answer).  Returns per problem (costs [N],
    clipped noise [H][N][nu], updated sequence [H][nu]) and the launch report."""
    from autompc_amd import _lib
    c = C.case(tag)
    nu = c["nu"]
    d = C.plan_data(tag, problems, cost)
    B = len(problems)
    h = _lib.Handle(0, precision)
    try:
        C.model(tag, precision).stage_into(h)
        h.set_quad_costs(d["Q"], d["R"], d["F"], d["goal"])
        if cost == "indicator":
            h.set_indicator_costs(C.indicator_terms(tag))
        h.set_ctrl_bounds(np.full(nu, C.LO), np.full(nu, C.HI))
        plan = _lib.MppiPlan(h, d["N"], d["H"], [C.SIGMA] * B, [C.LMDA] * B, cost_index=np.arange(B))
        plan.set_geometry(0, cap)
        launch = plan.sindy_launch()
        assert launch["lds_bytes"] <= C.LDS_LIMIT
        for k, v in (expect or {}).items():
            assert launch[k] == v, (tag, problems, k, launch)
        plan.upload(x0=d["x0"], act_seq=np.concatenate([a.ravel() for a in d["act"]]),
                    eps=np.concatenate([e.ravel() for e in d["eps"]]))
        plan.solve()
        a, _, cc, e = plan.download(act_seq=True, u=True, costs=True, eps_out=True)
        plan.close()
    finally:
        h.close()
    out, ao, co, eo = [], 0, 0, 0
    for N, H in problems:
        out.append((cc[co:co + N].copy(), e[eo:eo + N * H * nu].reshape(H, N, nu).copy(), a[ao:ao + H * nu].reshape(H, nu).copy()))
        ao, co, eo = ao + H * nu, co + N, eo + N * H * nu
    return out, launch


def _against_oracle(tag, problems, cost, expect, precision="f64", cap=C.HORIZON_CAP, tol=(1e-10, 1e-12, 1e-9), what=""):
    got, launch = _solve(tag, problems, cost, precision, cap, expect)
    worst = [0.0, 0.0, 0.0]
    for b, ((costs, eps, act), (o_costs, o_eps, o_act)) in enumerate(zip(got, C.cpu_rollouts(tag, problems, cost))):
        errs = rel_err(costs, o_costs), rel_err(eps, o_eps), rel_err(act, o_act)
        print("%s %s %s N %d H %d %s: costs %.2e clipped noise %.2e sequence %.2e"
              % ((tag, what, cost) + tuple(problems[b]) + (precision,) + errs))
        worst = [max(w, e) for w, e in zip(worst, errs)]
        assert errs[0] < tol[0] and errs[1] < tol[1] and errs[2] < tol[2], (tag, what, cost, problems[b])
    return got, launch


@pytest.mark.parametrize("mode", ["G16", "G32", "G64", "FP0"])
@pytest.mark.parametrize("tag", C.SPREAD_TAGS)
def test_lane_spread_rollouts_match_the_oracle(tag, mode, monkeypatch):
    """mppi_rollout_sindy_fp_kernel at G = 16, 32 (instantiated by no other test) and 64, and mppi_rollout_sindy_kernel
    on the same plans (AMPC_SINDY_FP=0: register accumulation at nx 5 .. 8 in the one-thread MPPI kernel), each with
    diagonal and dense Q / R / F (the cost_diag == 0 branch of the lane-spread kernel) and with indicator terms (its IND
    instantiations); N in (1, 5, 65, 130), H in (2, 8) under a cap of 8.  What the tags add:
      s5   5 states: the full-width reduction (nx > NR / 2); 78 features: the leftover loop past 2 G at G 16 / 32
      s8   8 states, 2 controls; 20 trig arguments: the second trig loop (j = g + G < n_trig) at G = 16; a power table
      s8w  6 controls; 28 trig arguments; 70 features: leftover at G = 32 only
      s6x  217 features: leftover at every G; powers and monomials formed by the lanes (n_pow, n_mon loops)
      s5p  12 features, no trig argument: lanes without a hoisted feature (fk false), t0 false in every lane
      s7 / s7t / s8t  32 / 64 / 128 features: exactly the hoisted 2 G at G = 16 / 32 / 64, so the leftover loop runs one
           side of each and not the other; s8t: 48 trig arguments (three rounds at G = 16), 8 controls
    Measured on MI355X (costs / updated sequence, worst over tags, costs and plans): 5.4e-16 / 4.1e-15 at G = 16,
    5.9e-16 / 2.1e-15 at G = 32 and at G = 64, 5.9e-16 / 5.8e-15 one thread per sample; clipped noise exact."""
    if mode == "FP0":
        monkeypatch.setenv("AMPC_SINDY_FP", "0")
        expect = dict(spread=False, lanes=1, staged=True)
    else:
        monkeypatch.setenv("AMPC_SINDY_G", mode[1:])
        expect = dict(spread=True, lanes=int(mode[1:]), staged=True)
    for cost in C.COSTS:
        for problems in C.PLANS:
            _against_oracle(tag, problems, cost, expect, what=mode)


@pytest.mark.parametrize("tag", C.THREAD_TAGS)
def test_one_thread_rollouts_match_the_oracle(tag):
    """mppi_rollout_sindy_kernel where the launcher must choose it by itself: s9 (nine states, a staged program: LDS
    accumulation), m40 (40 / 6, an unstaged 139-entry table), m56 (56 / 16, a power-only table, 157 KB of LDS) -- with
    diagonal, dense and indicator costs.  (t160 and max do not fit an f64 plan: test_refusals.)
    Measured on MI355X: costs <= 8.0e-16, updated sequence <= 2.3e-15."""
    expect = dict(spread=False, lanes=1, staged=tag == "s9")
    for cost in C.COSTS:
        for problems in C.PLANS:
            _against_oracle(tag, problems, cost, expect, what="one thread")


@pytest.mark.parametrize("n,h,lanes", C.NATURAL)
def test_the_launchers_own_choice_of_lanes(n, h, lanes, monkeypatch):
    """2048 < samples <= 8192 picks 32 lanes and more picks 16: an s5 plan of 2100 / 8200 samples reports that, is bit
    for bit the plan forced to that value, and matches the oracle."""
    problems = ((n, h),)
    monkeypatch.delenv("AMPC_SINDY_G", raising=False)
    got, _ = _against_oracle("s5", problems, "diag", dict(spread=True, lanes=lanes), cap=h, what="natural")
    monkeypatch.setenv("AMPC_SINDY_G", str(lanes))
    forced, _ = _solve("s5", problems, cap=h, expect=dict(spread=True, lanes=lanes))
    for x, y in zip(got[0], forced[0]):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("G", ["16", "64"])
@pytest.mark.parametrize("tag", ["s5", "s8"])
def test_lane_spread_rollouts_f32(tag, G, monkeypatch):
    """The f32 instantiations (sincosf, powf, 4-byte DPP moves) against the f64 oracle at 1e-4."""
    monkeypatch.setenv("AMPC_SINDY_G", G)
    for problems in C.PLANS:
        _against_oracle(tag, problems, "diag", dict(spread=True, lanes=int(G)), precision="f32", tol=(1e-4, 1e-4, 1e-4),
                        what="G" + G)


def test_the_fall_back_to_one_thread_when_the_lane_spread_map_does_not_fit(monkeypatch):
    """lbf > kLdsLimit at nx <= 8: s8w under a horizon cap of 1700 (tests/test_sindy_kernels_host.py derives it) reports
    and runs the one-thread kernel whatever AMPC_SINDY_G says; under the cap of 8 the same plan is lane-spread."""
    tag, cap = C.FALLBACK
    problems = ((5, 2), (65, 8))
    for G in (None, "16"):
        if G:
            monkeypatch.setenv("AMPC_SINDY_G", G)
        _against_oracle(tag, problems, "diag", dict(spread=False, lanes=1, staged=True), cap=cap, what="cap %d" % cap)
    _solve(tag, problems, expect=dict(spread=True, lanes=16))


def test_a_program_staged_for_prediction_runs_unstaged_in_the_rollout():
    """`lds` (30 / 8, a 48 048-byte program): pred_batch stages it (161 216 B, in test_pred_and_jacobian_*); the MPPI
    rollout's columns and cost block leave no room for it (177 072 B), so the plan reports and launches the one-thread
    kernel on the program in global memory, at 129 008 B -- and matches the oracle.  Before, plan creation passed and the
    launch asked for 177 072 B."""
    for cost in ("diag", "dense"):
        for problems in C.PLANS:
            _, launch = _against_oracle("lds", problems, cost, dict(spread=False, lanes=1, staged=False), what="unstaged")
            assert launch["lds_bytes"] == 129008


def test_refusals():
    """What does not fit is refused by name before any launch: f64 MPPI plans on t160 / max (columns + cost block beyond
    160 KB), a prediction whose columns and staged program exceed 160 KB (a raw descriptor list: 79 sin features on
    64 / 16), and more than 4096 features (46 variables with trig interaction: 4278)."""
    from autompc_amd import SINDy, _lib
    from helpers import make_system
    for tag in C.MPPI_REFUSED:
        c = C.case(tag)
        h = _lib.Handle(0, "f64")
        C.model(tag).stage_into(h)
        h.set_quad_costs(np.eye(c["nx"]), np.eye(c["nu"]), np.eye(c["nx"]), np.zeros(c["nx"]))
        h.set_ctrl_bounds(np.full(c["nu"], C.LO), np.full(c["nu"], C.HI))
        with pytest.raises(_lib.AmpcError, match="160 KB LDS"):
            _lib.MppiPlan(h, [5], [2], [C.SIGMA], [C.LMDA])
        h.close()
    nx, nu, nf = C.RAW_PRED_REFUSED[0], 16, C.RAW_PRED_REFUSED[1]
    h = _lib.Handle(0, "f64")
    var = np.arange(nf, dtype=np.int32)
    h.set_sindy(nx, nu, np.full(nf, 1, dtype=np.int32), var, var, np.full(nf, 2.0), 0.01 * np.ones((nx, nf)), False, C.DT)
    with pytest.raises(_lib.AmpcError, match="ampc_sindy_pred_batch.*staged feature program.*160 KB"):
        h.pred_batch(np.zeros((3, nx)), np.zeros((3, nu)))
    h.close()
    big = SINDy(make_system(45, 1), trig_basis=True, trig_freq=1, trig_interaction=True)
    assert big.coefficients.shape[1] == 4278
    with pytest.raises(_lib.AmpcError, match="n_feat in 1..4096"):
        big.pred_batch(np.zeros((1, 45)), np.zeros((1, 1)))


# ---- iLQR on the single-model path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("H", C.ILQR_H)
@pytest.mark.parametrize("tag", C.ILQR_TAGS)
def test_ilqr_matches_the_oracle(tag, H):
    """sindy_forward_kernel and sindy_jacobian_kernel through the iLQR plan's RowMap (rows of live problems only) at 5
    and 9 states, horizons 1 and 5, bounded controls: the oracle's decisions, states and controls 1e-7, gains 1e-6 (the
    bounds of test_gpu_sindy.py::test_ilqr_on_sindy_model_matches_oracle).
    Measured on MI355X: states <= 3.1e-16, controls <= 2.2e-15, gains <= 2.6e-15."""
    from autompc_amd import IterativeLQR, QuadCost, Task
    c = C.case(tag)
    system, p, ref = C.system(tag), C.ilqr_problem(tag), C.ilqr_oracle(tag, H)
    task = Task(system)
    task.set_cost(QuadCost(system, p["Q"], p["R"], p["F"]))
    task.set_ctrl_bounds(np.full(c["nu"], C.ILQR_BOUNDS[0]), np.full(c["nu"], C.ILQR_BOUNDS[1]))
    ctl = IterativeLQR(system, task, C.model(tag, strict=True), H)
    conv, states, ctrls, Ks, _ = ctl.compute_ilqr_default(np.array(p["x0"]), np.zeros((H, c["nu"])))
    errs = rel_err(states, ref["states"]), rel_err(ctrls, ref["ctrls"]), rel_err(Ks, ref["Ks"])
    print("%s iLQR H %d: converged %s iters %d; states %.2e ctrls %.2e gains %.2e"
          % ((tag, H, conv, ctl.last_iters) + errs))
    assert bool(conv) == ref["converged"] and ctl.last_iters == ref["iters"]
    assert errs[0] < 1e-7 and errs[1] < 1e-7 and errs[2] < 1e-6
