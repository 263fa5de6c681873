"""DifferentiableProgram on the device: Jacobians from the staged JVP program (program_jacobian_kernel) against the
host evaluation of the same JVP, what ampc_set_program_jvp refuses, and the program as an MPPI controller model
(csrc/mppi_program_kernels.hpp): solves against the oracle, the closed loop, the drop-in controller.  Needs MI355X.

Tolerances.  JVP programs of exactly rounded operations: device == host bit for bit, in f64 and f32.  JVP programs with
sin / cos / exp / tanh: the rule of test_gpu_program.py for values (1e-12 * max(1, |want|) in f64, 1e-5 in f32) -- a
JVP program is a program of the same operations on the same ranges.  MPPI solves against the oracle: the bounds of the
one-thread SINDy rollout (test_gpu_sindy.py:69-70: costs 1e-10, sequence and control 1e-9; test_gpu_mppi.py:92: clipped
noise 1e-12; :128 f32: costs 1e-4, sequence 1e-3) -- the same arithmetic around a different dynamics call.  Indicator
terms: test_gpu_indicator.py's 1e-9 / 1e-8.  Closed loop: 1e-7 (test_gpu_program.py)."""
import numpy as np
import pytest

import program_cases as C
import program_diff_cases as D
from autompc_amd import DifferentiableProgram, DynamicsProgram, _lib
from autompc_amd.sysid import program as P
from helpers import rel_err
from oracle.costs import BoxCostOracle, QuadCostOracle, SumCostOracle, ThresholdCostOracle
from oracle.mppi import MPPIOracle

pytestmark = pytest.mark.gpu
NP_T = {"f64": np.float64, "f32": np.float32}
ROWS = [1, 2, 13, 64, 65]


@pytest.fixture(scope="module")
def progs():
    p = D.traced(DifferentiableProgram)
    p["exact_n(1,1)"] = DifferentiableProgram.trace(C.system_of(1, 1), C.exact_n(1, 1))
    return p


def _host_jvp(prog, X, U, precision):
    return [a.astype(np.float64) for a in prog.evaluate_jvp(X, U, dtype=NP_T[precision])]


# ---- Jacobians -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", ["exact_fn", "exact_n(1,1)", "exact_n(17,6)"])
def test_exact_jvp_programs_equal_the_host_bit_for_bit(progs, name, precision):
    """nv = 5, 2 and 23 lanes per row: the (row, direction) lanes end on and run across workgroup edges."""
    prog = progs[name]
    nx, nu = prog.system.obs_dim, prog.system.ctrl_dim
    for n in ROWS:
        X, U = D.away_from_kinks(nx, nu, n, seed=n)
        got = prog.pred_diff_batch(X, U, device=True, precision=precision)
        want = _host_jvp(prog, X, U, precision)
        assert got[0].shape == (n, nx) and got[1].shape == (n, nx, nx) and got[2].shape == (n, nx, nu)
        for g, w in zip(got, want):
            assert np.all(np.isfinite(w)) and np.array_equal(g, w), (name, n)
        assert np.array_equal(got[0], prog.pred_batch(X, U, device=True, precision=precision))


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_kinks_and_powers_equal_the_host_bit_for_bit(precision):
    cases = [(make(DifferentiableProgram), X, U) for make, X, U in D.kink_rows()]
    a = np.array([[-1.5], [-0.5], [0.75], [1.25]])
    cases += [(D.powi_program(DifferentiableProgram, e), a, np.ones((4, 1))) for e in D.POWERS]
    for prog, X, U in cases:
        for n in ROWS:
            Xn, Un = np.resize(X, (n, X.shape[1])), np.resize(U, (n, U.shape[1]))
            got = prog.pred_diff_batch(Xn, Un, device=True, precision=precision)
            for g, w in zip(got, _host_jvp(prog, Xn, Un, precision)):
                assert np.all(np.isfinite(w)) and np.array_equal(g, w), (prog.code.tolist(), n)
    # the tangent at the kink itself: 0 for abs, a's for a tie of min / max
    _, jx, _ = cases[0][0].pred_diff_batch(cases[0][1], cases[0][2], device=True, precision=precision)
    assert np.array_equal(jx[:, 0, 0], [-2.0, 0.0, -0.5])
    _, jx, _ = cases[1][0].pred_diff_batch(cases[1][1], cases[1][2], device=True, precision=precision)
    assert np.array_equal(jx[2], [[3.0, 0.0], [3.0, 0.0]])


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", ["smooth_fn", "smooth_n(17,6)", "cartpole"])
def test_transcendental_jvp_programs_are_within_the_library_bound(progs, name, precision):
    prog = progs[name]
    nx, nu = prog.system.obs_dim, prog.system.ctrl_dim
    tol = 1e-12 if precision == "f64" else 1e-5
    worst = 0.0
    for n in (1, 65):
        X, U = D.away_from_kinks(nx, nu, n, seed=20 + n)
        got = prog.pred_diff_batch(X, U, device=True, precision=precision)
        for g, w in zip(got, _host_jvp(prog, X, U, precision)):
            assert np.all(np.isfinite(w))
            worst = max(worst, float((np.abs(g - w) / np.maximum(1.0, np.abs(w))).max()))
    print("JVP %s %s: largest |device - host| / max(1, |host|) = %.3e (bound %.0e)" % (name, precision, worst, tol))
    assert worst <= tol


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_jvp_of_exactly_256_slots(precision):
    nx, nu, n_slots, code, consts, out = D.jvp_at_slot_limit()
    h = _lib.Handle(0, precision)
    h.set_program(nx, nu, 3, [[P.OP_ADD, 2, 0, 1]], [], [2])
    h.set_program_jvp(n_slots, code, consts, out)
    X, U = D.away_from_kinks(1, 1, 65, seed=1)
    nxt, jx, ju = h.pred_diff_batch(X, U)
    T = NP_T[precision]
    V = np.concatenate([X, U, np.ones((65, 1)), np.zeros((65, 1))], axis=1)
    want = P.ProgramArrays(4, code, consts, out, n_slots).evaluate(V, T).astype(np.float64)
    assert np.array_equal(nxt[:, 0], want[:, 0]) and np.array_equal(jx[:, 0, 0], np.ones(65))
    assert np.array_equal(ju[:, 0, 0], np.ones(65))
    h.close()


# ---- the ABI ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_what_set_program_jvp_refuses(precision):
    h = _lib.Handle(0, precision)
    add = [P.OP_ADD, 2, 0, 1]
    jvp = dict(n_slots=5, code=[[P.OP_ADD, 4, 0, 1], [P.OP_ADD, 2, 2, 3]], consts=[], out=[4, 2])
    with pytest.raises(_lib.AmpcError, match="holds no program") as e:
        h.set_program_jvp(jvp["n_slots"], jvp["code"], jvp["consts"], jvp["out"])
    assert e.value.code != 0
    h.set_program(1, 1, 3, [add], [], [2])
    jadd = [P.OP_ADD, 4, 0, 1]
    bad = {
        "unknown opcode": dict(n_slots=5, code=[[17, 4, 0, 1]], consts=[], out=[4, 2]),
        "operand slot outside": dict(n_slots=5, code=[[P.OP_LT, 4, 0, 5]], consts=[], out=[4, 2]),
        "destination slot outside": dict(n_slots=5, code=[[P.OP_SIGN, 5, 0, 0]], consts=[], out=[0, 2]),
        "before anything wrote it": dict(n_slots=6, code=[[P.OP_ADD, 4, 0, 5]], consts=[], out=[4, 2]),
        "constant index outside": dict(n_slots=5, code=[[P.OP_CONST, 4, 1, 0]], consts=[1.0], out=[4, 2]),
        "names a slot nothing wrote": dict(n_slots=6, code=[jadd], consts=[], out=[4, 5]),
        "out_slot[1] outside": dict(n_slots=5, code=[jadd], consts=[], out=[4, 5]),
        "n_slots must cover the 4 input slots": dict(n_slots=3, code=[], consts=[], out=[0, 2]),
        "n_slots must cover": dict(n_slots=P.MAX_SLOTS + 1, code=[jadd], consts=[], out=[4, 2]),
        "instructions": dict(n_slots=5, code=[jadd] * (P.MAX_INSTR + 1), consts=[], out=[4, 2]),
        "exponent outside": dict(n_slots=5, code=[[P.OP_POWI, 4, 0, -65]], consts=[], out=[4, 2]),
    }
    for text, b in bad.items():
        with pytest.raises(_lib.AmpcError, match=text.replace("[", r"\[").replace("]", r"\]")) as e:
            h.set_program_jvp(b["n_slots"], b["code"], b["consts"], b["out"])
        assert e.value.code != 0 and "ampc_set_program_jvp" in str(e.value)
        with pytest.raises(_lib.AmpcError, match="no Jacobians"):          # a refused JVP stages nothing
            h.pred_diff_batch(np.array([[1.5]]), np.array([[0.25]]))
    # a well-formed one: Jacobians and MPPI plans; the iLQR and LQR plans still refuse
    h.set_program_jvp(jvp["n_slots"], jvp["code"], jvp["consts"], jvp["out"])
    nxt, jx, ju = h.pred_diff_batch(np.array([[1.5]]), np.array([[0.25]]))
    assert np.array_equal(nxt, [[1.75]]) and np.array_equal(jx, [[[1.0]]]) and np.array_equal(ju, [[[1.0]]])
    h.set_quad_costs(np.eye(1), np.eye(1), np.eye(1), np.zeros(1))
    h.set_ctrl_bounds([-1.0], [1.0])
    plan = _lib.MppiPlan(h, [16], 5, 0.5, 1.0)
    with pytest.raises(_lib.AmpcError, match="MLP models"):
        plan.set_models([h], [0])
    with pytest.raises(_lib.AmpcError, match="not a SINDy model"):
        plan.set_sindy_models([h], [0])
    with pytest.raises(_lib.AmpcError, match="not a linear model"):
        plan.set_linear_models([h], [0])
    with pytest.raises(_lib.AmpcError, match="state is the observation"):
        plan.set_state_lift([0], [0.0])
    plan.close()
    with pytest.raises(_lib.AmpcError, match="not a controller model"):
        _lib.IlqrPlan(h, 1, 5, 0.05)
    if precision == "f64":
        with pytest.raises(_lib.AmpcError, match="not a controller model"):
            _lib.LqrPlan([h], 1, 1)
    # set_program drops the JVP: today's refusals return, with today's texts
    h.set_program(1, 1, 3, [add], [], [2])
    with pytest.raises(_lib.AmpcError, match="no Jacobians"):
        h.pred_diff_batch(np.array([[1.5]]), np.array([[0.25]]))
    with pytest.raises(_lib.AmpcError, match="not a controller model"):
        _lib.MppiPlan(h, [16], 5, 0.5, 1.0)
    h.close()


# ---- MPPI solves against the oracle ----------------------------------------------------------------------------------
NH = [(1, 2), (65, 7), (130, 5)]              # one lane; a tile edge; two tiles and an idle tail


def _problems(name, prog):
    """Three problems with their own sigma, lmda, Q, R, F; bounds tight enough that the clipping is active."""
    nx, nu = prog.system.obs_dim, prog.system.ctrl_dim
    rng = np.random.default_rng(nx)
    B = len(NH)
    pr = dict(nx=nx, nu=nu, Ns=[n for n, _ in NH], Hs=[h for _, h in NH],
              sig=rng.uniform(0.3, 1.2, B), lam=rng.uniform(0.4, 1.5, B),
              Q=np.stack([np.diag(rng.uniform(0.5, 2.0, nx)) for _ in range(B)]),
              R=np.stack([np.diag(rng.uniform(0.05, 0.3, nu)) for _ in range(B)]),
              F=np.stack([np.diag(rng.uniform(0.5, 2.0, nx)) for _ in range(B)]),
              goal=rng.normal(scale=0.1, size=(B, nx)), lo=-rng.uniform(0.3, 0.6, nu), hi=rng.uniform(0.4, 0.7, nu),
              x0=rng.uniform(-0.5, 0.5, (B, nx)))
    pr["acts"] = [rng.normal(scale=0.3, size=(h, nu)) for h in pr["Hs"]]
    pr["eps"] = [rng.normal(scale=np.sqrt(pr["sig"][b]), size=(pr["Ns"][b], pr["Hs"][b], nu)) for b in range(B)]
    return pr


def _device_solve(prog, pr, which, precision, term_mode):
    """(per-problem costs, clipped noise [H][N][nu], sequence [H][nu], control) of the problems `which` in one plan."""
    nu = pr["nu"]
    h = _lib.Handle(0, precision)
    prog.stage_into(h)
    h.set_quad_costs(pr["Q"], pr["R"], pr["F"], pr["goal"])
    h.set_ctrl_bounds(pr["lo"], pr["hi"])
    plan = _lib.MppiPlan(h, [pr["Ns"][b] for b in which], [pr["Hs"][b] for b in which], pr["sig"][which], pr["lam"][which],
                         cost_index=np.asarray(which), term_mode=term_mode)
    plan.upload(pr["x0"][which], np.concatenate([pr["acts"][b].ravel() for b in which]),
                np.concatenate([pr["eps"][b].ravel() for b in which]))
    plan.solve()
    a, u, c, e = plan.download(costs=True, eps_out=True)
    out, ao, co, eo = [], 0, 0, 0
    for k, b in enumerate(which):
        N, H = pr["Ns"][b], pr["Hs"][b]
        out.append((c[co:co + N].copy(), e[eo:eo + N * H * nu].reshape(H, N, nu).copy(),
                    a[ao:ao + H * nu].reshape(H, nu).copy(), u[k].copy()))
        ao, co, eo = ao + H * nu, co + N, eo + N * H * nu
    plan.close()
    h.close()
    return out


@pytest.fixture(scope="module")
def solved(progs):
    """Device solves (f64, both terminal modes) and the oracle's, once per controller model."""
    out = {}
    for name in ("cartpole", "exact_n(17,6)"):
        prog = progs[name]
        pr = _problems(name, prog)
        ref = {}
        for term in (_lib.TERM_REFERENCE, _lib.TERM_PER_PARTICLE):
            ref[term] = []
            for b in range(len(NH)):
                orc = MPPIOracle(prog, QuadCostOracle(pr["Q"][b], pr["R"][b], pr["F"][b], pr["goal"][b]),
                                 np.stack([pr["lo"], pr["hi"]], axis=1), horizon=pr["Hs"][b], num_path=pr["Ns"][b],
                                 sigma=pr["sig"][b], lmda=pr["lam"][b],
                                 per_particle_terminal=term == _lib.TERM_PER_PARTICLE)
                orc.act_sequence = pr["acts"][b].copy()
                u, _ = orc.run(np.concatenate([pr["x0"][b], np.zeros(pr["nu"])]), pr["x0"][b], eps_nhu=pr["eps"][b])
                ref[term].append((orc.last_costs.copy(), orc.last_eps.copy(), orc.act_sequence.copy(), u.copy()))
        dev = {term: _device_solve(prog, pr, [0, 1, 2], "f64", term) for term in ref}
        out[name] = dict(prog=prog, pr=pr, ref=ref, dev=dev)
    return out


@pytest.mark.parametrize("term", [_lib.TERM_REFERENCE, _lib.TERM_PER_PARTICLE])
@pytest.mark.parametrize("name", ["cartpole", "exact_n(17,6)"])
def test_mppi_solve_matches_the_oracle(solved, name, term):
    S = solved[name]
    clipped = False
    for b, ((c, e, a, u), (oc, oe, oa, ou)) in enumerate(zip(S["dev"][term], S["ref"][term])):
        errs = (rel_err(c, oc), rel_err(e, oe), rel_err(a, oa), rel_err(u, ou))
        print("%s term %d problem %d: costs %.2e eps %.2e sequence %.2e control %.2e" % ((name, term, b) + errs))
        assert errs[0] < 1e-10 and errs[1] < 1e-12 and errs[2] < 1e-9 and errs[3] < 1e-9
        clipped = clipped or not np.allclose(oe, S["pr"]["eps"][b].transpose(1, 0, 2))
    assert clipped                                     # the bounds did cut samples


@pytest.mark.parametrize("name", ["cartpole", "exact_n(17,6)"])
def test_mppi_solve_in_f32_agrees_with_f64(solved, name):
    S = solved[name]
    got = _device_solve(S["prog"], S["pr"], [0, 1, 2], "f32", _lib.TERM_REFERENCE)
    for (c, e, a, u), (dc, de, da, du) in zip(got, S["dev"][_lib.TERM_REFERENCE]):
        assert rel_err(c, dc) < 1e-4 and rel_err(a, da) < 1e-3 and rel_err(u, du) < 1e-3


def test_a_problem_does_not_depend_on_its_place_in_the_batch(solved):
    S = solved["cartpole"]
    term = _lib.TERM_REFERENCE
    want = S["dev"][term][1]
    alone = _device_solve(S["prog"], S["pr"], [1], "f64", term)[0]
    first = _device_solve(S["prog"], S["pr"], [1, 0, 2], "f64", term)[0]
    last = _device_solve(S["prog"], S["pr"], [2, 0, 1], "f64", term)[2]
    for got in (alone, first, last):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


def test_indicator_cost_terms_vs_oracle(progs):
    """Threshold and box terms in the controller's cost (the IND instantiation), the drop-in MPPI against the oracle."""
    from autompc_amd import MPPI, BoxThresholdCost, QuadCost, Task, ThresholdCost
    prog = progs["cartpole"]
    system, no = prog.system, 4
    rng = np.random.default_rng(4)
    Q, F, R = np.diag(rng.uniform(0.5, 2, no)), np.diag(rng.uniform(0.5, 2, no)), np.diag(rng.uniform(0.01, 0.1, 1))
    goal = rng.normal(scale=0.05, size=no)
    limits = np.stack([goal - rng.uniform(0.05, 0.3, no), goal + rng.uniform(0.05, 0.3, no)], axis=1)
    limits[0, 0], limits[no - 1, 1] = -np.inf, np.inf
    task = Task(system)
    task.set_cost(QuadCost(system, Q, R, F, goal=goal) + ThresholdCost(system, goal, [1, 3], 0.12)
                  + BoxThresholdCost(system, limits))
    task.set_ctrl_bounds([-1.0], [1.0])
    ocost = SumCostOracle([QuadCostOracle(Q, R, F, goal), ThresholdCostOracle(goal, [1, 3], 0.12), BoxCostOracle(limits)])
    np.random.seed(3)
    orc = MPPIOracle(prog, ocost, np.array([[-1.0, 1.0]]), horizon=9, num_path=96, sigma=0.7, lmda=0.9)
    np.random.seed(3)
    ctl = MPPI(system, task, prog, horizon=9, num_path=96, sigma=0.7, lmda=0.9)
    x = rng.uniform(-0.2, 0.2, no)
    cs = np.concatenate([x, np.zeros(1)])
    levels = set()
    for _ in range(2):
        st = np.random.get_state()
        uo, _ = orc.run(cs, x)
        np.random.set_state(st)
        uh, _ = ctl.run(cs, x, return_details=True)
        assert rel_err(ctl.last_costs, orc.last_costs) < 1e-9
        assert rel_err(ctl.act_sequence, orc.act_sequence) < 1e-8 and rel_err(uh, uo) < 1e-8
        ctl.act_sequence = orc.act_sequence
        levels |= set(np.round(orc.last_costs).astype(int).tolist())
    assert len(levels) > 2                              # the indicator terms tell samples apart


# ---- closed loop, drop-in controller ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop(progs):
    system = C.cartpole_system()
    return dict(system=system, task=C.loop_task(system), ctl=progs["cartpole"],
                sim=DynamicsProgram.trace(system, C.cartpole_step))


def test_closed_loop_on_the_program_matches_the_oracle_stepped_on_the_host(loop):
    from autompc_amd.trajectory import Trajectory
    from autompc_amd.tuning import CandidateEvaluator
    cands, T = C.mppi_cands(), C.LOOP_STEPS
    acts, eps = C.mppi_noise(cands, T)
    eps_all = np.concatenate([np.concatenate([e.ravel() for e in step]) for step in eps])
    ev = CandidateEvaluator(loop["system"], loop["task"], loop["ctl"], surrogate=loop["sim"])
    kw = dict(n_steps=T, init_obs=C.LOOP_INIT, eps_all=eps_all, act_init=np.concatenate([a.ravel() for a in acts]))
    scores, obs, ctrls = ev.evaluate(cands, return_trajectories=True, **kw)
    ref = D.oracle_program_loops(loop["sim"], cands, acts, eps, T)
    cost = loop["task"].get_cost()
    for b, (o_obs, o_ctl) in enumerate(ref):
        assert rel_err(obs[b], o_obs) < 1e-7 and rel_err(ctrls[b], o_ctl) < 1e-7
        # every recorded row is the device program's own one-step prediction of the row before
        assert np.array_equal(obs[b, 1:], loop["sim"].pred_batch(obs[b, :-1], ctrls[b, :-1], device=True)), b
        want = cost(Trajectory(loop["system"], T + 1, obs[b].copy(), ctrls[b].copy()))
        assert abs(scores[b] - want) < 1e-10 * max(1.0, abs(want))
    assert np.any(ctrls != 0.0)


def test_closed_loop_with_device_noise_repeats_and_tuner_takes_the_evaluator(loop):
    from autompc_amd.tuning import BatchPipelineTuner, CandidateEvaluator
    ev = CandidateEvaluator(loop["system"], loop["task"], loop["ctl"], surrogate=loop["sim"])
    cands = C.mppi_cands()
    scores = ev.evaluate(cands, seed=3)
    assert np.all(np.isfinite(scores))
    np.testing.assert_array_equal(scores, ev.evaluate(cands, seed=3))
    pool = C.mppi_cands()
    tuner = BatchPipelineTuner(loop["system"], ev, batch_size=3, sampler=lambda n, rng: [pool.pop(0) for _ in range(n)],
                               truedyn_evaluator=ev)
    _, res = tuner.run(3, np.random.default_rng(0), seed=3)
    np.testing.assert_array_equal(res.truedyn_costs, scores)
    # a plain DynamicsProgram as controller model fails in the library, as before
    with pytest.raises(_lib.AmpcError, match="not a controller model"):
        CandidateEvaluator(loop["system"], loop["task"], loop["sim"]).evaluate(cands, seed=3)


def test_drop_in_mppi_on_the_program_matches_the_oracle(loop):
    from autompc_amd import MPPI
    prog, kw = loop["ctl"], dict(horizon=8, num_path=100, sigma=0.6, lmda=0.8)
    bounds = np.array([[-C.LOOP_UMAX, C.LOOP_UMAX]])
    ocost = QuadCostOracle(np.eye(4), 0.1 * np.eye(1), 2.0 * np.eye(4), np.zeros(4))
    assert MPPI.is_compatible(loop["system"], loop["task"], prog)
    np.random.seed(5)
    ctl = MPPI(loop["system"], loop["task"], prog, **kw)
    np.random.seed(5)
    orc = MPPIOracle(prog, ocost, bounds, **kw)
    obs = C.LOOP_INIT.copy()
    cs_h = cs_o = np.concatenate([obs, np.zeros(1)])
    for k in range(3):
        st = np.random.get_state()
        uo, cs_o = orc.run(cs_o, obs)
        np.random.set_state(st)
        uh, cs_h = ctl.run(cs_h, obs, return_details=(k == 0))       # the detailed call, then the one-call step
        if k == 0:
            assert rel_err(ctl.last_costs, orc.last_costs) < 1e-10
        assert rel_err(ctl.act_sequence, orc.act_sequence) < 1e-9 and rel_err(uh, uo) < 1e-9
        ctl.act_sequence = orc.act_sequence
        obs = prog.pred(obs, uo)
    np.random.seed(6)
    ctl.reset()
    np.random.seed(6)
    orc.reset()
    assert np.array_equal(ctl.act_sequence, orc.act_sequence) and ctl.cur_step == 0


# ---- the LDS limit ----------------------------------------------------------------------------------------------------
def test_a_program_whose_slots_do_not_fit_lds_is_refused_in_f64_and_runs_in_f32():
    code, consts, out, jcode, jout = D.wide_state_program()
    nx, nu = 64, 1
    rng = np.random.default_rng(0)
    Q, R, F = np.diag(rng.uniform(0.5, 2.0, nx)), 0.1 * np.eye(1), np.eye(nx)
    handles = {}
    for precision in ("f64", "f32"):
        h = handles[precision] = _lib.Handle(0, precision)
        h.set_program(nx, nu, P.MAX_SLOTS, code, consts, out)
        h.set_program_jvp(P.MAX_SLOTS, jcode, consts, jout)
        h.set_quad_costs(Q, R, F, np.zeros(nx))
        h.set_ctrl_bounds([-1.0], [1.0])
    with pytest.raises(_lib.AmpcError, match="256 program slots, 64 states.*160 KB"):
        _lib.MppiPlan(handles["f64"], [70], 4, 0.5, 1.0)
    plan = _lib.MppiPlan(handles["f32"], [70], 4, 0.5, 1.0)
    x0, act, eps = rng.uniform(-0.5, 0.5, (1, nx)), rng.normal(scale=0.3, size=(4, 1)), rng.normal(scale=0.7, size=(70, 4, 1))
    plan.upload(x0, act, eps)
    plan.solve()
    a, u, c, _ = plan.download(costs=True)
    prog = DynamicsProgram.from_code(C.system_of(nx, nu), code, consts, out, n_slots=P.MAX_SLOTS)
    orc = MPPIOracle(prog, QuadCostOracle(Q, R, F, np.zeros(nx)), np.array([[-1.0, 1.0]]), horizon=4, num_path=70,
                     sigma=0.5, lmda=1.0)
    orc.act_sequence = act.copy()
    uo, _ = orc.run(np.concatenate([x0[0], np.zeros(1)]), x0[0], eps_nhu=eps)
    assert rel_err(c, orc.last_costs) < 1e-4 and rel_err(a.reshape(4, 1), orc.act_sequence) < 1e-3
    assert rel_err(u[0], uo) < 1e-3
    plan.close()
    for h in handles.values():
        h.close()
