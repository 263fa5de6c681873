"""iLQR on analytic dynamics programs (ampc_program_set_ilqr): the perfect-model iLQR plan.  Needs MI355X.

The line search runs the interpreter on one column per candidate row (csrc/ilqr_kernels.hpp, DYN = 3), the Jacobian
refresh runs the JVP on one lane per (plan row, input direction) (csrc/program_kernels.hpp).  The reference is
oracle.ilqr.ILQROracle on the DifferentiableProgram's host methods with QuadCostOracle; the cases, their inputs and
the margins of the oracle's decisions are in program_ilqr_cases.py (asserted without a GPU by
test_program_ilqr_host.py).

Tolerances, the project's own: solves as test_ilqr_on_sindy_model_matches_oracle (states and controls 1e-7, gains
1e-6, rel_err); program values and Jacobians inside the plan array_equal to the device's own batched calls for
programs of exactly rounded operations and within test_gpu_program.py's value rule (1e-12 * max(1, |want|))
otherwise; closed loops 1e-7 (test_gpu_program.py)."""
import numpy as np
import pytest

import program_cases as C
import program_ilqr_cases as K
from autompc_amd import DifferentiableProgram, DynamicsProgram, _lib
from autompc_amd.sysid import program as P
from helpers import rel_err

pytestmark = pytest.mark.gpu
CASES = K.solve_cases()
NAMES = ("cartpole", "poly_step", "exact_n(17,6)", "smooth_n(62,1)", "smooth_n(53,1)")


@pytest.fixture(scope="module")
def progs():
    return {name: K.program(name) for name in NAMES}


def _handle(prog, Q, R, F, bounds=None, precision="f64"):
    h = _lib.Handle(0, precision)
    prog.stage_into(h)
    nx = prog.system.obs_dim
    Q = np.asarray(Q)
    h.set_quad_costs(Q, R, F, np.zeros(Q.shape[:-2] + (nx,)))
    if bounds is not None:
        h.set_ctrl_bounds(*bounds)
    return h


def _case_plan(prog, case):
    nx, nu = prog.system.obs_dim, prog.system.ctrl_dim
    q, r, f = K.quad(nx, nu)
    ub = K.ubounds(case, nu)
    h = _handle(prog, q, r, f if case.get("F") is None else case["F"], ub)
    try:
        return h, _lib.IlqrPlan(h, 1, case["H"], prog.system.dt, clip_to_bounds=ub is not None)
    except _lib.AmpcError:
        h.close()
        raise


@pytest.fixture(scope="module")
def solved(progs):
    """Every case once: the device solve, the oracle's, and the open plan (shared, left unchanged)."""
    out = {}
    for cid, case in CASES.items():
        prog = progs[case["prog"]]
        h, plan = _case_plan(prog, case)
        orc = K.case_oracle(prog, case)
        out[cid] = dict(case=case, prog=prog, h=h, plan=plan, orc=orc,
                        dev=plan.solve(case["x0"][None], case["guess"][None], case["max_iter"]),
                        ref=orc.solve(case["x0"], case["guess"]))
    yield out
    for s in out.values():
        s["plan"].close()
        s["h"].close()


def _close(got, want):
    return np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))


# ---- solves against the oracle ---------------------------------------------------------------------------------------
def _check_solve(cid, s):
    dev, (oc, ost, oct_, oKs, oks), orc = s["dev"], s["ref"], s["orc"]
    assert dev["status"][0] == 0
    assert bool(dev["converged"][0]) == bool(oc) and int(dev["iters"][0]) == orc.n_iter
    e = (rel_err(dev["states"][0], ost), rel_err(dev["ctrls"][0], oct_), rel_err(dev["Ks"][0], oKs))
    print(cid, "iters", orc.n_iter, "rel_err states %.3g ctrls %.3g Ks %.3g" % e)
    assert e[0] < 1e-7 and e[1] < 1e-7 and e[2] < 1e-6
    assert abs(dev["objective"][0] - orc.final_obj) < 1e-9 * max(1.0, abs(orc.final_obj))
    steps = K.device_step_indices(s["plan"], orc, s["case"]["x0"], s["case"]["guess"], orc.n_iter)
    want = orc.step_indices()
    assert len(steps) == len(want) and all(w in got for got, w in zip(steps, want)), (steps, want)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_solve_matches_the_oracle(solved, cid):
    _check_solve(cid, solved[cid])


# ---- the interpreter inside the plan ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c for c in sorted(CASES) if c[0] in "ABC"])
def test_nominal_trajectory_and_jacobians_are_the_devices_own(solved, cid):
    """states[t + 1] is the device program's prediction of (states[t], ctrls[t]) -- after the solve (rows swapped in by
    the line search) and after the rollout of the guess alone (max_iter = 0: the r == 0 lane of row 0) -- and the plan's
    Jacobian rows are Handle.pred_diff_batch's on the trajectory they were refreshed on: the guess's after max_iter = 0,
    the first accepted candidate's after max_iter = 1 where the solve goes on after it."""
    s = solved[cid]
    prog, plan, case = s["prog"], s["plan"], s["case"]
    exact = case["prog"] in K.EXACT
    same = np.array_equal if exact else _close
    for out in (s["dev"], plan.solve(case["x0"][None], case["guess"][None], 0)):
        st, ct = out["states"][0], out["ctrls"][0]
        assert np.array_equal(st[0], case["x0"])
        assert same(st[1:], prog.pred_batch(st[:-1], ct, device=True)), cid
    assert np.array_equal(ct, case["guess"])
    for k in (0, 1):
        out = plan.solve(case["x0"][None], case["guess"][None], k)
        if k == 1 and out["converged"][0]:
            continue
        jx, ju = plan.jacobians()
        _, wx, wu = prog.pred_diff_batch(out["states"][0][:-1], out["ctrls"][0], device=True)
        assert jx.shape == (1,) + wx.shape and ju.shape == (1,) + wu.shape
        assert same(jx[0], wx) and same(ju[0], wu), (cid, k)
        if not exact:
            print(cid, k, "max |jx - want| %.3g |ju - want| %.3g" % (np.abs(jx[0] - wx).max(), np.abs(ju[0] - wu).max()))


# ---- determinism and the row map -------------------------------------------------------------------------------------
H3 = 7
X3 = np.array([[0.3, -0.2, 0.1, 0.0], [0.01, 0.0, -0.01, 0.0], [-0.4, 0.3, 0.2, -0.1]])
Q3 = np.stack([np.eye(4), np.diag([2.0, 1.0, 0.5, 1.0]), np.diag([1.0, 3.0, 1.0, 0.25])])
R3 = np.stack([0.1 * np.eye(1), 0.3 * np.eye(1), 0.05 * np.eye(1)])
F3 = np.stack([5.0 * np.eye(4), 2.0 * np.eye(4), 8.0 * np.eye(4)])
KEYS = ("states", "ctrls", "Ks", "ks", "converged", "iters", "status", "objective")


@pytest.fixture(scope="module")
def three(progs):
    """Three CartPole problems with different costs and x0, each solved alone (the reference of this section); the
    oracle takes 5, 2 and 7 iterations on them."""
    prog = progs["cartpole"]
    h = _handle(prog, Q3, R3, F3)
    alone = []
    for k in range(3):
        plan = _lib.IlqrPlan(h, 1, H3, C.DT, cost_index=[k])
        alone.append(plan.solve(X3[k][None], np.zeros((1, H3, 1))))
        plan.close()
    assert [int(a["iters"][0]) for a in alone] == [5, 2, 7]       # (they retire at different iterations)
    yield dict(prog=prog, h=h, alone=alone)
    h.close()


def test_problems_give_the_same_bits_alone_in_a_batch_and_at_any_slot(three):
    h, alone = three["h"], three["alone"]
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        plan = _lib.IlqrPlan(h, 3, H3, C.DT, cost_index=order)
        out = plan.solve(X3[order], np.zeros((3, H3, 1)))
        plan.close()
        for slot, k in enumerate(order):
            for key in KEYS:
                assert np.array_equal(out[key][slot], alone[k][key][0]), (order, slot, key)


def test_queue_with_per_problem_horizons_gives_the_same_bits(three):
    h = three["h"]
    hz, prob = [2, 7, 1, 7, 4], [0, 1, 2, 2, 0]
    plan = _lib.IlqrPlan(h, 2, H3, C.DT)
    out = plan.solve_queue(X3[prob], None, prob, horizon=hz)
    plan.close()
    for j, (H, k) in enumerate(zip(hz, prob)):
        one = _lib.IlqrPlan(h, 1, H, C.DT, cost_index=[k])
        ref = one.solve(X3[k][None], np.zeros((1, H, 1)))
        one.close()
        for key in ("converged", "iters", "status", "objective"):
            assert np.array_equal(out[key][j], ref[key][0]), (j, key)
        assert np.array_equal(out["states"][j][:H + 1], ref["states"][0]) and np.all(out["states"][j][H + 1:] == 0.0)
        for key in ("ctrls", "Ks", "ks"):
            assert np.array_equal(out[key][j][:H], ref[key][0]) and np.all(out[key][j][H:] == 0.0), (j, key)


def test_refresh_leaves_the_rows_of_retired_slots_and_past_the_horizon_alone(three):
    """(a) A slot that retires early keeps the Jacobian rows of its last refresh while the others iterate on: problem 1
    converges first; its rows after the whole batch has finished are, bit for bit, those after one iteration fewer
    than it took (the iteration that retires a slot does not refresh it).  (b) Rows poisoned through the read-back stay
    poisoned where the row map says nothing lives: the slot of a queue that never got a problem, and the rows past a
    slot's horizon."""
    h, alone = three["h"], three["alone"]
    n = [int(a["iters"][0]) for a in alone]
    assert n[1] >= 2 and n[1] < max(n)
    plan = _lib.IlqrPlan(h, 3, H3, C.DT, cost_index=[0, 1, 2])
    plan.solve(X3, np.zeros((3, H3, 1)), n[1] - 1)
    jx_before, ju_before = plan.jacobians()
    plan.solve(X3, np.zeros((3, H3, 1)))
    jx, ju = plan.jacobians()
    assert np.array_equal(jx[1], jx_before[1]) and np.array_equal(ju[1], ju_before[1])
    assert not np.array_equal(jx[0], jx_before[0])               # (the others went on and were refreshed)
    plan.close()
    plan = _lib.IlqrPlan(h, 2, H3, C.DT)
    poison_x, poison_u = np.full((2, H3, 4, 4), -7.25), np.full((2, H3, 4, 1), -7.25)
    plan.set_jacobians(poison_x, poison_u)
    out = plan.solve_queue(X3[:1], None, [0], horizon=[3])       # one problem of horizon 3 through two slots
    jx, ju = plan.jacobians()
    plan.close()
    assert out["iters"][0] >= 1
    b = 0 if jx[0, 0, 0, 0] != -7.25 else 1                       # (whichever idle slot took the problem)
    assert np.all(jx[1 - b] == -7.25) and np.all(ju[1 - b] == -7.25)       # the idle slot
    assert np.all(jx[b, 3:] == -7.25) and np.all(ju[b, 3:] == -7.25)       # past the horizon
    assert np.all(jx[b, :3] != -7.25) and np.all(np.isfinite(jx[b, :3])) and np.all(ju[b, :3] != -7.25)


# ---- closed loop and drop-in -----------------------------------------------------------------------------------------
def _ilqr_cands():
    return [dict(horizon=6 + b, Q=np.full(4, 1.0 + b), R=np.full(1, 0.1 * (1 + b)), F=np.full(4, 2.0)) for b in range(4)]


@pytest.fixture(scope="module")
def loop(progs):
    system = progs["cartpole"].system
    return dict(system=system, task=C.loop_task(system), ctl=progs["cartpole"],
                sim=DynamicsProgram.trace(system, C.cartpole_step))


@pytest.mark.parametrize("umax", [C.LOOP_UMAX, 6.0])
def test_closed_loop_matches_the_oracle_stepped_on_the_host(loop, umax):
    """loop_task as it is (bounds +-1.5: on these candidates every control of the episode sits on the bound, on both
    sides) and with bounds +-6, where every control is interior (-4.2 .. -2.2, 4-5 iterations per solve)."""
    from autompc_amd.tuning import IlqrCandidateEvaluator
    from oracle.costs import QuadCostOracle
    from oracle.ilqr import ILQROracle
    prog, sim, cands, T = loop["ctl"], loop["sim"], _ilqr_cands(), C.LOOP_STEPS
    task = C.loop_task(loop["system"])
    task.set_ctrl_bounds([-umax], [umax])
    ev = IlqrCandidateEvaluator(loop["system"], task, prog, surrogate=sim)
    scores, obs, ctrls = ev.evaluate(cands, n_steps=T, init_obs=C.LOOP_INIT, return_trajectories=True)
    assert obs.shape == (4, T + 1, 4) and np.all(np.isfinite(scores)) and np.any(ctrls != 0.0)
    assert np.all(np.abs(ctrls[:, :-1]) == umax) if umax == C.LOOP_UMAX else np.all(np.abs(ctrls) < umax)
    np.testing.assert_array_equal(scores, ev.evaluate(cands, n_steps=T, init_obs=C.LOOP_INIT))
    ub = (np.array([-umax]), np.array([umax]))
    for b, c in enumerate(cands):
        # every row is the device program's own prediction of the row before
        assert np.array_equal(obs[b, 1:], sim.pred_batch(obs[b, :-1], ctrls[b, :-1], device=True)), b
        orc = ILQROracle(prog, QuadCostOracle(np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), np.zeros(4)), C.DT,
                         c["horizon"], ubounds=ub)
        x, cs = C.LOOP_INIT.copy(), np.concatenate([C.LOOP_INIT, np.zeros(1)])
        o_obs, o_ctl = [x.copy()], []
        for _ in range(T):
            u, cs = orc.run(cs, x)
            x = sim.pred(x, u)
            o_ctl.append(u)
            o_obs.append(x.copy())
        o_ctl.append(np.zeros(1))
        e = (rel_err(obs[b], np.array(o_obs)), rel_err(ctrls[b], np.array(o_ctl)))
        print("umax", umax, "candidate", b, "rel_err obs %.3g ctrls %.3g" % e)
        assert e[0] < 1e-7 and e[1] < 1e-7


def test_closed_loop_against_an_mlp_surrogate_is_finite_and_repeats(loop):
    from autompc_amd import MLP
    from autompc_amd.tuning import IlqrCandidateEvaluator
    p = C.loop_mlp_params()
    m = MLP(loop["system"], n_hidden_layers=len(p["weights"]) - 1, nonlintype=p["activation"],
            **{"hidden_size_%d" % (i + 1): w.shape[0] for i, w in enumerate(p["weights"][:-1])})
    m.weights, m.biases = [w.copy() for w in p["weights"]], [b.copy() for b in p["biases"]]
    m.xu_means, m.xu_std, m.dy_means, m.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
    ev = IlqrCandidateEvaluator(loop["system"], loop["task"], loop["ctl"], surrogate=m)
    scores, obs, ctrls = ev.evaluate(_ilqr_cands(), return_trajectories=True)
    assert np.all(np.isfinite(scores)) and np.all(np.isfinite(obs)) and np.any(ctrls != 0.0)
    np.testing.assert_array_equal(scores, ev.evaluate(_ilqr_cands()))


def test_tuner_takes_the_evaluator_for_its_true_dynamics_column(loop):
    from autompc_amd.tuning import BatchPipelineTuner, IlqrCandidateEvaluator
    ev = IlqrCandidateEvaluator(loop["system"], loop["task"], loop["ctl"], surrogate=loop["sim"])
    scores = ev.evaluate(_ilqr_cands())
    pool = _ilqr_cands()
    tuner = BatchPipelineTuner(loop["system"], ev, batch_size=4, sampler=lambda n, rng: [pool.pop(0) for _ in range(n)],
                               truedyn_evaluator=ev)
    _, res = tuner.run(4, np.random.default_rng(0))
    np.testing.assert_array_equal(res.truedyn_costs, scores)


def test_drop_in_controller_matches_the_oracle(solved):
    from autompc_amd import IterativeLQR
    s = solved["A-H15-bounded"]
    prog, case = s["prog"], s["case"]
    ctl = IterativeLQR(prog.system, K.case_task(prog, case), prog, 15)
    conv, states, ctrls, Ks, ks = ctl.compute_ilqr_default(case["x0"], case["guess"])
    for key, got in (("states", states), ("ctrls", ctrls), ("Ks", Ks), ("ks", ks)):
        assert np.array_equal(got, s["dev"][key][0]), key         # (the plan of the solve cases, through the class)
    assert conv == bool(s["ref"][0]) and ctl.last_iters == s["orc"].n_iter
    orc = K.case_oracle(prog, case)
    for again in range(2):
        x, cs, co = case["x0"].copy(), np.concatenate([case["x0"], np.zeros(1)]), np.concatenate([case["x0"], np.zeros(1)])
        for _ in range(3):
            u, cs = ctl.run(cs, x)
            uo, co = orc.run(co, x)
            assert rel_err(u, uo) < 1e-7 and rel_err(cs, co) < 1e-7
            x = prog.pred(x, uo)
        ctl.reset()
        orc.reset()


# ---- refusals --------------------------------------------------------------------------------------------------------
def _refused(call, text):
    with pytest.raises(_lib.AmpcError, match=text) as e:
        call()
    assert e.value.code != 0


def _raw(nx, nu, n_slots=None, cls=DifferentiableProgram, **kw):
    """x_i' = x_i + u_(i mod nu), in place: nx + nu slots unless n_slots names more."""
    code = [[P.OP_ADD, i, i, nx + i % nu] for i in range(nx)]
    return cls.from_code(C.system_of(nx, nu), code, [], list(range(nx)), n_slots=n_slots or nx + nu, **kw)


def test_the_opt_in_needs_a_program_with_its_jvp_and_every_model_call_clears_it(progs):
    prog = progs["cartpole"]
    h = _lib.Handle(0, "f64")
    _refused(h.set_program_ilqr, "ampc_program_set_ilqr: the handle holds no analytic dynamics program")
    p = C.loop_mlp_params()
    mlp = (4, 1, p["weights"], p["biases"], p["activation"], p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"])
    h.set_mlp(*mlp)
    _refused(h.set_program_ilqr, "ampc_program_set_ilqr: the handle holds no analytic dynamics program")
    DynamicsProgram.stage_into(prog, h)                            # the program alone
    _refused(h.set_program_ilqr, "ampc_program_set_ilqr: the handle's program has no JVP staged")
    h.set_quad_costs(np.eye(4), 0.1 * np.eye(1), 5.0 * np.eye(4), np.zeros(4))
    jvp = (prog.jvp.n_slots, prog.jvp.code, prog.jvp.consts, prog.jvp.out_slot)
    h.set_program_jvp(*jvp)
    _refused(lambda: _lib.IlqrPlan(h, 1, 5, C.DT), "not a controller model")       # the JVP alone: as before
    h.set_program_ilqr()
    plan = _lib.IlqrPlan(h, 1, 5, C.DT)
    x0, guess = K.X0_A[None], np.zeros((1, 5, 1))
    first = plan.solve(x0, guess)
    h.set_program_ilqr(False)
    _refused(lambda: _lib.IlqrPlan(h, 1, 5, C.DT), "not a controller model")
    _refused(lambda: plan.solve(x0, guess), "call ampc_program_set_ilqr again")
    h.set_program_ilqr()
    # set_program_jvp clears it: no new plan, and the plan built before refuses to solve until it is set again
    h.set_program_jvp(*jvp)
    _refused(lambda: _lib.IlqrPlan(h, 1, 5, C.DT), "not a controller model")
    _refused(lambda: plan.solve(x0, guess), "call ampc_program_set_ilqr again")
    _refused(lambda: plan.solve_queue(x0), "call ampc_program_set_ilqr again")
    _refused(lambda: plan.closed_loop(x0, 2), "call ampc_program_set_ilqr again")
    h.set_program_ilqr()
    again = plan.solve(x0, guess)
    assert all(np.array_equal(first[k], again[k]) for k in KEYS)
    # set_program clears it together with the JVP
    DynamicsProgram.stage_into(prog, h)
    _refused(lambda: plan.solve(x0, guess), "call ampc_program_set_ilqr again")
    _refused(h.set_program_ilqr, "no JVP staged")
    h.set_program_jvp(*jvp)
    _refused(lambda: _lib.IlqrPlan(h, 1, 5, C.DT), "not a controller model")
    h.set_program_ilqr()
    # set_mlp clears it: the plan sees another model; the program staged again starts without the flag
    h.set_mlp(*mlp)
    _refused(lambda: plan.solve(x0, guess), "its handle holds another model now")
    DynamicsProgram.stage_into(prog, h)
    h.set_program_jvp(*jvp)
    _refused(lambda: _lib.IlqrPlan(h, 1, 5, C.DT), "not a controller model")
    _refused(lambda: plan.solve(x0, guess), "call ampc_program_set_ilqr again")
    prog.stage_into(h)
    again = plan.solve(x0, guess)
    assert all(np.array_equal(first[k], again[k]) for k in KEYS)
    plan.close()
    h.close()


def test_a_plan_built_on_another_model_refuses_a_program_staged_under_it(progs):
    p = C.loop_mlp_params()
    h = _lib.Handle(0, "f64")
    h.set_mlp(4, 1, p["weights"], p["biases"], p["activation"], p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"])
    h.set_quad_costs(np.eye(4), 0.1 * np.eye(1), 5.0 * np.eye(4), np.zeros(4))
    plan = _lib.IlqrPlan(h, 1, 5, C.DT)
    first = plan.solve(K.X0_A[None], np.zeros((1, 5, 1)))
    progs["cartpole"].stage_into(h)
    _refused(lambda: plan.solve(K.X0_A[None], np.zeros((1, 5, 1))), "built before its handle held an analytic dynamics program")
    h.set_mlp(4, 1, p["weights"], p["biases"], p["activation"], p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"])
    again = plan.solve(K.X0_A[None], np.zeros((1, 5, 1)))
    assert all(np.array_equal(first[k], again[k]) for k in KEYS)
    plan.close()
    h.close()


def test_plan_creation_refuses_what_the_kernels_are_not_built_for(progs):
    prog = progs["cartpole"]
    h = _handle(prog, np.eye(4), 0.1 * np.eye(1), 5.0 * np.eye(4), precision="f32")
    _refused(lambda: _lib.IlqrPlan(h, 1, 5, C.DT), "built for f64 handles; this program's handle is f32")
    h.close()
    wide = _raw(48, 16, ilqr=True)                                 # nx + nu = 64
    h = _handle(wide, np.eye(48), np.eye(16), np.eye(48))
    _refused(lambda: _lib.IlqrPlan(h, 1, 3, C.DT), "state dim \\+ ctrl dim must be <= 63")
    h.close()
    h = _handle(prog, np.eye(4), 0.1 * np.eye(1), 5.0 * np.eye(4))
    h.set_indicator_costs((np.array([2], dtype=np.int32), np.concatenate([-np.ones(4), np.ones(4)])))
    _refused(lambda: _lib.IlqrPlan(h, 1, 5, C.DT), "indicator terms")
    h.set_indicator_costs(None)
    _lib.IlqrPlan(h, 1, 5, C.DT).close()
    # the default DifferentiableProgram -- the JVP without the flag -- still is no iLQR controller model
    DifferentiableProgram.trace(prog.system, C.cartpole_step).stage_into(h)
    _refused(lambda: _lib.IlqrPlan(h, 1, 5, C.DT), "not a controller model")
    h.close()


def test_a_plan_past_the_full_map_runs_on_the_compact_one_with_the_same_bits():
    """45 states and 8 controls: rows 16 * 54, next states 16 * 45, the full workspace 15235 values (its cost block 4252)
    and 16 values per slot -- 8 * (16819 + 16 s) bytes.  228 slots are 163 736 bytes, inside the 163 840 of a workgroup:
    the full map.  229 are 163 864: the compact map (80 424 bytes) and the sweep that reads its cost block from global
    memory (87 864 bytes).  The two programs are the same instructions, so the two tiers must give the same bits.
    No program inside ampc_set_program's limits can be over the compact tier (at 256 slots the largest requests are
    113 304 and 128 368 bytes: test_program_ilqr_host.py walks every nx + nu <= 63), so the refusal that names the
    program's slots has no instance to test; what is refused is a program larger than the plan was built for."""
    cs = K.cost_block_stride(45, 8)
    assert K.plan_lds_bytes(45, 8, 228, cs) == 163736 and K.plan_lds_bytes(45, 8, 229, cs) == 163864
    assert K.plan_compact_bytes(45, 8, 229, cs) == (80424, 87864)
    Q, R = np.eye(45), np.eye(8)
    x0, guess = np.linspace(-0.2, 0.2, 45), np.full((1, 3, 8), 0.1)
    outs = []
    for n_slots in (228, 229, 256):
        prog = _raw(45, 8, n_slots, ilqr=True)
        h = _handle(prog, Q, R, 5.0 * Q, (np.full(8, -0.3), np.full(8, 0.3)))
        plan = _lib.IlqrPlan(h, 1, 3, C.DT, clip_to_bounds=True)
        outs.append(plan.solve(x0[None], guess))
        if n_slots == 228:
            jx, ju = plan.jacobians()
        else:
            jx2, ju2 = plan.jacobians()
            assert np.array_equal(jx, jx2) and np.array_equal(ju, ju2)
        plan.close()
        h.close()
    assert outs[0]["status"][0] == 0 and outs[0]["iters"][0] >= 1
    st, ct = outs[0]["states"][0], outs[0]["ctrls"][0]
    assert np.array_equal(st[1:], prog.pred_batch(st[:-1], ct))
    for o in outs[1:]:
        assert all(np.array_equal(o[k], outs[0][k]) for k in KEYS)
    # a larger program staged after the plan was built: refused at solve
    fits = _raw(45, 8, 228, ilqr=True)
    h = _handle(fits, Q, R, Q)
    plan = _lib.IlqrPlan(h, 1, 2, C.DT)
    plan.solve(x0[None], np.zeros((1, 2, 8)), 1)
    _raw(45, 8, 229, ilqr=True).stage_into(h)
    _refused(lambda: plan.solve(x0[None], np.zeros((1, 2, 8)), 2), "has 229 value slots, the plan's LDS map was built for 228")
    _raw(44, 8, 60, ilqr=True).stage_into(h)
    _refused(lambda: plan.solve(x0[None, :44], np.zeros((1, 2, 8)), 2), "other dimensions than the one the plan was built for")
    plan.close()
    h.close()


def test_tables_and_model_index_are_refused_on_such_a_plan(solved, progs):
    s = solved["A-H2-free"]
    plan, h2 = s["plan"], _lib.Handle(0, "f64")
    progs["cartpole"].stage_into(h2)
    p = C.loop_mlp_params()
    from autompc_amd import MLP
    m = MLP(s["prog"].system, n_hidden_layers=2, nonlintype=p["activation"], hidden_size_1=32, hidden_size_2=32)
    m.weights, m.biases = [w.copy() for w in p["weights"]], [b.copy() for b in p["biases"]]
    m.xu_means, m.xu_std, m.dy_means, m.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
    text = "the plan's controller model is an analytic dynamics program"
    _refused(lambda: plan.set_models([h2]), "ampc_ilqr_plan_set_models: " + text)
    _refused(lambda: plan.set_model_table([m]), "ampc_ilqr_plan_set_model_table: " + text)
    _refused(lambda: plan.set_sindy_models([h2]), "ampc_ilqr_plan_set_sindy_models: " + text)
    _refused(lambda: plan.set_linear_models([h2]), "ampc_ilqr_plan_set_linear_models: " + text)
    x0 = s["case"]["x0"][None]
    _refused(lambda: plan.solve_queue(x0, model_index=[0]), "ampc_ilqr_solve_queue_var: model_index given: " + text)
    _refused(lambda: plan.closed_loop(x0, 2, model_index=[0]), "ampc_ilqr_closed_loop_var: model_index given: " + text)
    again = plan.solve(x0, s["case"]["guess"][None])               # the plan is as it was
    assert all(np.array_equal(again[k], s["dev"][k]) for k in KEYS)
    _refused(lambda: _lib.LqrPlan([s["h"]], 1, 1), "not a controller model")
    h2.close()


def test_without_the_flag_the_classes_fail_in_the_library_as_before(loop):
    from autompc_amd import IterativeLQR
    from autompc_amd.tuning import IlqrCandidateEvaluator
    plain = DifferentiableProgram.trace(loop["system"], C.cartpole_step)          # the JVP, not the flag
    h = _lib.Handle(0, "f64")
    plain.stage_into(h)
    h.set_quad_costs(np.eye(4), 0.1 * np.eye(1), 5.0 * np.eye(4), np.zeros(4))
    _refused(lambda: _lib.IlqrPlan(h, 1, 5, C.DT), "not a controller model")
    h.close()
    ctl = IterativeLQR(loop["system"], loop["task"], plain, 5)
    _refused(lambda: ctl.compute_ilqr_default(C.LOOP_INIT, np.zeros((5, 1))), "not a controller model")
    ev = IlqrCandidateEvaluator(loop["system"], loop["task"], plain, surrogate=loop["sim"])
    _refused(lambda: ev.evaluate(_ilqr_cands()), "not a controller model")
