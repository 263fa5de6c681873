"""DynamicsProgram on the device (csrc/program_kernels.hpp): one step and rollouts against the host evaluation of the
same instruction list, what ampc_set_program refuses, and the program as the simulation model of the MPPI, iLQR and
LQR closed loops and of the tuner's true-dynamics column.  Needs MI355X.

Tolerances.  Programs of add / sub / mul / div / sqrt / abs / min / max / integer power only: device == host bit for
bit, in f64 and in f32 (the host then evaluates in np.float32).  Programs with sin / cos / exp / tanh: one step within
1e-12 * max(1, |x|) in f64 -- the device library's double-precision elementary functions are within 4 ulp ~ 9e-16,
carried through <= 30 operations on magnitudes <= ~20, which leaves more than 10x margin -- and 1e-5 in f32 (4 ulp of
f32 by the same count).  A rollout row t+1 is the device's own one-step prediction of row t bit for bit."""
import os

import numpy as np
import pytest

import program_cases as C
from autompc_amd import DynamicsProgram, System, Task, data_generation
from autompc_amd.sysid import program as P

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCHES = [1, 63, 64, 65, 130]                      # block edges and an idle tail
NP_T = {"f64": np.float64, "f32": np.float32}


def _inputs(nx, nu, B, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, (B, nx)), rng.uniform(-2.0, 2.0, (B, nu))


def _host(prog, X, U, precision):
    return prog.evaluate(X, U, dtype=NP_T[precision]).astype(np.float64)


def _close(got, want, precision):
    tol = 1e-12 if precision == "f64" else 1e-5
    assert np.all(np.isfinite(want))
    assert np.all(np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want))), np.abs(got - want).max()


@pytest.fixture(scope="module")
def programs():
    return {(name, nx, nu): DynamicsProgram.trace(C.system_of(nx, nu), make(nx, nu))
            for name, make in (("exact", C.exact_n), ("smooth", C.smooth_n)) for nx, nu in ((1, 1), (17, 6))}


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("dims", [(1, 1), (17, 6)])
def test_exact_arithmetic_programs_equal_the_host_bit_for_bit(programs, dims, precision):
    progs = [programs[("exact",) + dims]]
    if dims == (1, 1):
        progs.append(DynamicsProgram.trace(C.system_of(3, 2), C.exact_fn))      # every exact op, a*b+c, powers
    for prog in progs:
        nx, nu = prog.system.obs_dim, prog.system.ctrl_dim
        for B in BATCHES:
            X, U = _inputs(nx, nu, B, seed=B)
            got = prog.pred_batch(X, U, device=True, precision=precision)
            assert got.shape == (B, nx)
            assert np.array_equal(got, _host(prog, X, U, precision)), (nx, nu, B)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("dims", [(1, 1), (17, 6)])
def test_transcendental_programs_are_within_the_library_bound(programs, dims, precision):
    progs = [programs[("smooth",) + dims]]
    if dims == (1, 1):
        progs += [DynamicsProgram.trace(C.system_of(3, 2), C.smooth_fn),
                  DynamicsProgram.trace(C.cartpole_system(), C.cartpole_step)]
    for prog in progs:
        nx, nu = prog.system.obs_dim, prog.system.ctrl_dim
        for B in (1, 65, 130):
            X, U = _inputs(nx, nu, B, seed=10 + B)
            _close(prog.pred_batch(X, U, device=True, precision=precision), _host(prog, X, U, precision), precision)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_programs_at_the_slot_and_instruction_limits(precision):
    system = C.system_of(1, 1)
    X, U = _inputs(1, 1, 65, seed=3)
    at_slots = DynamicsProgram.trace(system, C.wide(P.MAX_SLOTS - 1))
    at_instr = DynamicsProgram.trace(system, C.chain(P.MAX_INSTR))
    assert at_slots.n_slots == P.MAX_SLOTS and at_instr.code.shape[0] == P.MAX_INSTR
    for prog in (at_slots, at_instr):
        assert np.array_equal(prog.pred_batch(X, U, device=True, precision=precision), _host(prog, X, U, precision))
    # the rollout of the widest program asks for the slots plus the hand-over rows
    obs = at_slots.rollout(X, np.repeat(U[:, None, :], 2, axis=1), device=True, precision=precision)
    assert np.array_equal(obs[:, 1], _host(at_slots, X, U, precision))


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_raw_programs_passthrough_constant_output_and_dst_equal_to_an_operand(precision):
    system = C.system_of(2, 1)
    X, U = _inputs(2, 1, 65, seed=4)
    # outputs that ARE input slots, swapped
    swap = DynamicsProgram.from_code(system, np.zeros((0, 4), np.int32), [], [1, 0])
    assert np.array_equal(swap.pred_batch(X, U, device=True, precision=precision), X[:, ::-1].astype(NP_T[precision]))
    # a constant output, and dst == a: slot 0 = slot 0 + slot 2, in place
    prog = DynamicsProgram.from_code(system, [[P.OP_CONST, 3, 0, 0], [P.OP_ADD, 0, 0, 2], [P.OP_MUL, 0, 0, 0]],
                                     [0.1], [0, 3])
    want = _host(prog, X, U, precision)
    assert np.array_equal(want[:, 1], np.full(65, NP_T[precision](0.1), dtype=np.float64))
    assert np.array_equal(prog.pred_batch(X, U, device=True, precision=precision), want)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_rollout_of_a_swap_program_reads_nothing_already_overwritten(precision):
    """x0' = x1, x1' = x0 + u: output 0 is an input slot and the outputs permute the inputs."""
    system = C.system_of(2, 1)
    prog = DynamicsProgram.from_code(system, [[P.OP_ADD, 3, 0, 2]], [], [1, 3])
    X, _ = _inputs(2, 1, 65, seed=5)
    U = np.random.default_rng(6).uniform(-1, 1, (65, 5, 1))
    got = prog.rollout(X, U, device=True, precision=precision)
    want = np.empty((65, 6, 2))
    want[:, 0] = X.astype(NP_T[precision])
    for t in range(5):
        want[:, t + 1] = _host(prog, want[:, t], U[:, t], precision)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 2, 0], (X[:, 0].astype(NP_T[precision]) + U[:, 0, 0].astype(NP_T[precision])))


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("n,T", [(1, 1), (1, 8), (65, 1), (65, 8)])
def test_rollout_rows_are_the_devices_own_one_step_predictions(programs, n, T, precision):
    for key in (("smooth", 17, 6), ("exact", 1, 1)):
        prog = programs[key]
        nx, nu = key[1], key[2]
        X, _ = _inputs(nx, nu, n, seed=7)
        U = np.random.default_rng(8).uniform(-2, 2, (n, T, nu))
        obs = prog.rollout(X, U, device=True, precision=precision)
        assert obs.shape == (n, T + 1, nx) and np.array_equal(obs[:, 0], X.astype(NP_T[precision]))
        for t in range(T):
            assert np.array_equal(obs[:, t + 1], prog.pred_batch(obs[:, t], U[:, t], device=True,
                                                                 precision=precision)), (key, t)
    # no steps: the initial rows alone
    assert np.array_equal(prog.rollout(X, np.zeros((n, 0, 1)), device=True), X[:, None, :])


def test_generators_match_the_reference_through_the_device_rollout():
    system, task = C.pendulum_system_task(System, Task)
    prog = DynamicsProgram.trace(system, C.pendulum2)
    cases = C.generator_cases(data_generation, system, task, prog, device=True)
    for name, trajs in cases.items():
        g = np.load(os.path.join(GOLDEN, "datagen_%s.npz" % name))
        assert [len(t) for t in trajs] == g["lens"].tolist(), name
        for k, t in enumerate(trajs):
            n = len(t)
            assert np.array_equal(t.ctrls, g["ctrls"][k, :n]), name
            want = g["obs"][k, :n]
            assert np.all(np.abs(t.obs - want) <= C.TRAJ_LEN * 1e-12 * np.maximum(1.0, np.abs(want))), name


# ---- what the library refuses: a return code and a message, never a launch -----------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_malformed_programs_are_refused_on_the_host(precision):
    from autompc_amd import _lib
    h = _lib.Handle(0, precision)
    add = [P.OP_ADD, 2, 0, 1]
    bad = {
        "unknown opcode": dict(n_slots=3, code=[[99, 2, 0, 1]], consts=[], out=[2]),
        "operand slot outside": dict(n_slots=3, code=[[P.OP_ADD, 2, 0, 3]], consts=[], out=[2]),
        "destination slot outside": dict(n_slots=3, code=[[P.OP_ADD, 3, 0, 1]], consts=[], out=[0]),
        "before anything wrote it": dict(n_slots=4, code=[[P.OP_ADD, 2, 0, 3]], consts=[], out=[2]),
        "constant index outside": dict(n_slots=3, code=[[P.OP_CONST, 2, 1, 0]], consts=[1.0], out=[2]),
        "names a slot nothing wrote": dict(n_slots=4, code=[add], consts=[], out=[3]),
        "out_slot[0] outside": dict(n_slots=3, code=[add], consts=[], out=[3]),
        "n_slots must cover": dict(n_slots=P.MAX_SLOTS + 1, code=[add], consts=[], out=[2]),
        "instructions": dict(n_slots=3, code=[add] * (P.MAX_INSTR + 1), consts=[], out=[2]),
        "exponent outside": dict(n_slots=3, code=[[P.OP_POWI, 2, 0, 65]], consts=[], out=[2]),
    }
    for text, b in bad.items():
        with pytest.raises(_lib.AmpcError, match=text.replace("[", r"\[").replace("]", r"\]")) as e:
            h.set_program(1, 1, b["n_slots"], b["code"], b["consts"], b["out"])
        assert e.value.code != 0
    with pytest.raises(_lib.AmpcError, match="holds no program"):
        h.program_rollout(np.zeros((1, 1)), np.zeros((1, 2, 1)))
    # a well-formed one after all that: the handle works, has no Jacobians and takes no plans
    h.set_program(1, 1, 3, [add], [], [2])
    assert np.array_equal(h.pred_batch(np.array([[1.5]]), np.array([[0.25]])), [[1.75]])
    with pytest.raises(_lib.AmpcError, match="no Jacobians"):
        h.pred_diff_batch(np.array([[1.5]]), np.array([[0.25]]))
    with pytest.raises(_lib.AmpcError, match="not a controller model"):
        _lib.MppiPlan(h, [16], 5, 0.5, 1.0)
    with pytest.raises(_lib.AmpcError, match="not a controller model"):
        _lib.IlqrPlan(h, 1, 5, 0.05)
    if precision == "f64":
        with pytest.raises(_lib.AmpcError, match="not a controller model"):
            _lib.LqrPlan([h], 1, 1)
    h.close()


# ---- the program as the simulation model of the closed loops -----------------------------------------------------
def _mlp(system, p):
    from autompc_amd import MLP
    m = MLP(system, n_hidden_layers=len(p["weights"]) - 1, nonlintype=p["activation"],
            **{"hidden_size_%d" % (i + 1): w.shape[0] for i, w in enumerate(p["weights"][:-1])})
    m.weights, m.biases = [w.copy() for w in p["weights"]], [b.copy() for b in p["biases"]]
    m.xu_means, m.xu_std, m.dy_means, m.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
    return m


def _arx(system, prog, task):
    from autompc_amd import ARX
    trajs = data_generation.uniform_random_generate(system, task, prog, np.random.default_rng(1), [-0.5] * 4,
                                                    [0.5] * 4, 30, 6)
    m = ARX(system, history=1)
    m.train(trajs)
    return m


def _ilqr_cands():
    return [dict(horizon=6 + b, Q=np.full(4, 1.0 + b), R=np.full(1, 0.1 * (1 + b)), F=np.full(4, 2.0)) for b in range(4)]


def _lqr_cands(model):
    return [dict(controller="lqr", finite_horizon=True, horizon=5 + 3 * b, Q=np.full(4, 1.0 + b), R=np.full(1, 0.5),
                 F=np.full(4, 1.0), model=model) for b in range(3)]


@pytest.fixture(scope="module")
def loop():
    system = C.cartpole_system()
    return dict(system=system, task=C.loop_task(system), mlp=_mlp(system, C.loop_mlp_params()),
                cart=DynamicsProgram.trace(system, C.cartpole_step), poly=DynamicsProgram.trace(system, C.poly_step))


def _evaluator(kind, S, prog, task=None, **kw):
    from autompc_amd.tuning import CandidateEvaluator, IlqrCandidateEvaluator, LqrCandidateEvaluator
    task = task or S["task"]
    if kind == "mppi":
        return CandidateEvaluator(S["system"], task, S["mlp"], surrogate=prog, **kw), C.mppi_cands()
    if kind == "ilqr":
        return IlqrCandidateEvaluator(S["system"], task, S["mlp"], surrogate=prog, **kw), _ilqr_cands()
    arx = _arx(S["system"], prog, task)
    return LqrCandidateEvaluator(S["system"], task, arx, surrogate=prog, **kw), _lqr_cands(arx)


def _check_rows(S, prog, scores, obs, ctrls, lengths=None):
    """Every recorded row is the device program's prediction of the row before; scores are the task cost of the rows."""
    from autompc_amd.trajectory import Trajectory
    cost = S["task"].get_cost()
    for b in range(obs.shape[0]):
        L = int(lengths[b]) if lengths is not None else obs.shape[1]
        assert np.all(np.isfinite(obs[b, :L])) and np.all(ctrls[b, L - 1] == 0.0)
        assert np.array_equal(obs[b, 1:L], prog.pred_batch(obs[b, :L - 1], ctrls[b, :L - 1], device=True)), b
        ref = cost(Trajectory(S["system"], L, obs[b, :L].copy(), ctrls[b, :L].copy()))
        assert abs(scores[b] - ref) < 1e-10 * max(1.0, abs(ref))


@pytest.mark.parametrize("kind", ["mppi", "ilqr", "lqr"])
@pytest.mark.parametrize("which", ["cart", "poly"])
def test_closed_loop_rows_are_the_programs_predictions(loop, kind, which):
    ev, cands = _evaluator(kind, loop, loop[which])
    scores, obs, ctrls = ev.evaluate(cands, seed=3, return_trajectories=True)
    assert obs.shape[:2] == (len(cands), C.LOOP_STEPS) and np.all(np.isfinite(scores))
    _check_rows(loop, loop[which], scores, obs, ctrls)
    assert np.any(ctrls != 0.0)
    np.testing.assert_array_equal(scores, ev.evaluate(cands, seed=3))


def test_mppi_closed_loop_matches_the_oracle_stepped_on_the_host(loop):
    """Explicit noise, the oracle MPPI on the host with the program as the dynamics (the pattern and the 1e-7 of
    test_gpu_closed_loop.py; test_program_host.py shows the oracle loop moves < 1e-9 under last-bit changes)."""
    from helpers import rel_err
    from autompc_amd.tuning import CandidateEvaluator
    prog, cands, T = loop["cart"], C.mppi_cands(), C.LOOP_STEPS
    acts, eps = C.mppi_noise(cands, T)
    eps_all = np.concatenate([np.concatenate([e.ravel() for e in step]) for step in eps])
    ev = CandidateEvaluator(loop["system"], loop["task"], loop["mlp"], surrogate=prog)
    scores, obs, ctrls = ev.evaluate(cands, n_steps=T, init_obs=C.LOOP_INIT, eps_all=eps_all,
                                     act_init=np.concatenate([a.ravel() for a in acts]), return_trajectories=True)
    ref = C.oracle_mppi_loops(loop["system"], C.loop_mlp_params(), cands, acts, eps, T, prog.pred)
    for b, (o_obs, o_ctl) in enumerate(ref):
        assert rel_err(obs[b], o_obs) < 1e-7 and rel_err(ctrls[b], o_ctl) < 1e-7


def test_ilqr_candidates_match_truedyn_score_on_the_host(loop):
    """The batched device loop against the parent's only way: BatchPipelineTuner.truedyn_score, the drop-in
    controller under simulate() with the (exact-arithmetic) program as the host dynamics."""
    from autompc_amd.tuning import BatchPipelineTuner
    ev, cands = _evaluator("ilqr", loop, loop["poly"])
    scores = ev.evaluate(cands)
    tuner = BatchPipelineTuner(loop["system"], ev)
    for b, c in enumerate(cands):
        ref = tuner.truedyn_score(c, loop["poly"])
        assert abs(scores[b] - ref) < 1e-7 * abs(ref), (b, scores[b], ref)


@pytest.mark.parametrize("kind", ["mppi", "ilqr"])
def test_user_termination_condition_runs_in_segments_on_the_program(loop, kind):
    task = C.loop_task(loop["system"], term_cond=lambda traj: len(traj) >= 4 and abs(traj[-1].obs[1]) > 0.05)
    kw = dict(term_check_every=3) if kind == "mppi" else {}
    ev, cands = _evaluator(kind, loop, loop["cart"], task=task, **kw)
    scores, obs, ctrls = ev.evaluate(cands, seed=5, return_trajectories=True)
    lengths = ev.last_lengths
    assert np.all(lengths >= 4) and np.all(lengths <= C.LOOP_STEPS + 1)
    _check_rows(loop, loop["cart"], scores, obs, ctrls, lengths)


def test_model_table_with_the_program_as_surrogate(loop):
    from autompc_amd.tuning import CandidateEvaluator
    other = _mlp(loop["system"], C.loop_mlp_params(seed=6, hidden=(48,)))
    cands = C.mppi_cands()
    cands[1]["model"] = other                              # mixed shapes: the table path
    ev = CandidateEvaluator(loop["system"], loop["task"], loop["mlp"], surrogate=loop["cart"], mlp_models="table")
    scores, obs, ctrls = ev.evaluate(cands, seed=2, return_trajectories=True)
    _check_rows(loop, loop["cart"], scores, obs, ctrls)


def test_tuner_fills_the_true_dynamics_column_on_the_device(loop):
    from autompc_amd.tuning import BatchPipelineTuner, CandidateEvaluator
    ev = CandidateEvaluator(loop["system"], loop["task"], loop["mlp"])
    true = CandidateEvaluator(loop["system"], loop["task"], loop["mlp"], surrogate=loop["cart"])
    pool = C.mppi_cands() + C.mppi_cands()
    tuner = BatchPipelineTuner(loop["system"], ev, batch_size=4, sampler=lambda n, rng: [pool.pop(0) for _ in range(n)],
                               truedyn_evaluator=true, keep_trajs=True)
    cands = list(pool)
    best, res = tuner.run(6, np.random.default_rng(0), seed=11)
    assert len(res.costs) == len(res.truedyn_costs) == len(res.truedyn_trajs) == len(res.surr_trajs) == 6
    assert np.all(np.isfinite(res.truedyn_costs))
    want = np.concatenate([true.evaluate(cands[:4], seed=11, index_offset=0),
                           true.evaluate(cands[4:], seed=11, index_offset=4)])
    np.testing.assert_array_equal(res.truedyn_costs, want)
    assert res.truedyn_costs != res.costs
    rows, ctl = res.truedyn_trajs[0]
    assert np.array_equal(np.array(rows)[1:], loop["cart"].pred_batch(np.array(rows)[:-1], np.array(ctl)[:-1],
                                                                     device=True))
    with pytest.raises(ValueError):
        tuner.run(1, np.random.default_rng(0), truedyn=loop["cart"])
