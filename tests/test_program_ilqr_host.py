"""The iLQR opt-in of DifferentiableProgram on the host (no GPU): the flag through every constructor, pickling, the
order of the staging calls -- and the inputs of the device tests: the oracle alone must keep MARGIN between everything
it decides on and its thresholds, in every iteration of every solve case (program_ilqr_cases.py)."""
import pickle

import numpy as np
import pytest

import program_cases as C
import program_ilqr_cases as K
from autompc_amd import DifferentiableProgram, DynamicsProgram


class Recorder:
    """Stands in for _lib.Handle: the staging calls, in order."""

    def __init__(self):
        self.calls = []

    def set_program(self, nx, nu, n_slots, code, consts, out_slot):
        self.calls.append(("set_program", nx, nu, n_slots))

    def set_program_jvp(self, n_slots, code, consts, out_slot):
        self.calls.append(("set_program_jvp", n_slots))

    def set_program_ilqr(self, enable=True):
        self.calls.append(("set_program_ilqr", enable))


def test_flag_through_every_constructor():
    system = C.cartpole_system()
    plain = DynamicsProgram.trace(system, C.cartpole_step)
    assert not hasattr(plain, "ilqr_plans")
    d = plain.differentiable()
    assert d.ilqr_plans is False
    assert plain.differentiable(ilqr=True).ilqr_plans is True
    assert DifferentiableProgram.trace(system, C.cartpole_step).ilqr_plans is False
    t = DifferentiableProgram.trace(system, C.cartpole_step, ilqr=True)
    assert t.ilqr_plans is True and t.differentiable() is t and t.differentiable(ilqr=True) is t
    f = DifferentiableProgram.from_code(system, t.code, t.consts, t.out_slot, ilqr=True)
    assert f.ilqr_plans is True and np.array_equal(f.jvp.code, t.jvp.code)
    assert DifferentiableProgram.from_code(system, t.code, t.consts, t.out_slot).ilqr_plans is False
    assert DifferentiableProgram(system, t.code, t.consts, t.out_slot, t.n_slots, ilqr=True).ilqr_plans is True
    # the flag changes nothing else: same arrays, same host results; a default program asked for it gives a copy
    e = d.differentiable(ilqr=True)
    assert e is not d and e.ilqr_plans and not d.ilqr_plans and np.array_equal(e.code, d.code)
    x, u = np.array([0.3, -0.2, 0.1, 0.0]), np.array([0.25])
    for a, b in zip(e.pred_diff(x, u), d.pred_diff(x, u)):
        assert np.array_equal(a, b)
    with pytest.raises(TypeError):
        DynamicsProgram.trace(system, C.cartpole_step, ilqr=True)      # (a plain program has no such option)


def test_pickle_keeps_the_flag_and_drops_the_handles():
    for flag in (False, True):
        p = DifferentiableProgram.trace(C.cartpole_system(), C.cartpole_step, ilqr=flag)
        p._handles["f64"] = object()           # (what a device call would have cached)
        state = p.__getstate__()
        assert state["_handles"] == {} and state["ilqr_plans"] is flag
        p._handles.clear()
        q = pickle.loads(pickle.dumps(p))
        assert q.ilqr_plans is flag and q._handles == {} and np.array_equal(q.jvp.code, p.jvp.code)


def test_stage_into_calls_program_then_jvp_then_flag():
    p = DifferentiableProgram.trace(C.cartpole_system(), C.cartpole_step, ilqr=True)
    h = Recorder()
    p.stage_into(h)
    assert h.calls == [("set_program", 4, 1, p.n_slots), ("set_program_jvp", p.jvp.n_slots), ("set_program_ilqr", True)]


def test_programs_without_the_flag_never_ask_for_it():
    system = C.cartpole_system()
    for p in (DynamicsProgram.trace(system, C.cartpole_step), DifferentiableProgram.trace(system, C.cartpole_step),
              DynamicsProgram.trace(system, C.cartpole_step).differentiable()):
        h = Recorder()
        p.stage_into(h)
        assert [c[0] for c in h.calls] == ["set_program", "set_program_jvp"][:len(h.calls)]
        assert all(c[0] != "set_program_ilqr" for c in h.calls)
    old = DifferentiableProgram.trace(system, C.cartpole_step)
    del old.__dict__["ilqr_plans"]             # (an object pickled before the option existed)
    h = Recorder()
    old.stage_into(h)
    assert [c[0] for c in h.calls] == ["set_program", "set_program_jvp"]


# What the oracle does on the chosen inputs: (iterations, converged, largest step index, clipping active)
EXPECT = {
    "A-H1-free": (2, True, 0, False), "A-H1-bounded": (2, True, 0, False),
    "A-H2-free": (2, True, 0, False), "A-H2-bounded": (2, True, 9, True),
    "A-H15-free": (5, True, 0, False), "A-H15-bounded": (3, True, 9, True),
    "B-H15": (2, True, 0, False),
    "C-H3-free": (11, True, 6, False), "C-H3-bounded": (11, True, 7, True),
    "C-H9-free": (15, True, 6, False), "C-H9-bounded": (14, True, 6, True),
    "D-H4": (3, False, 2, False), "E-H4": (3, False, 1, False),
}


@pytest.fixture(scope="module")
def programs():
    return {name: K.program(name) for name in ("cartpole", "poly_step", "exact_n(17,6)", "smooth_n(62,1)",
                                               "smooth_n(53,1)")}


@pytest.mark.parametrize("cid", sorted(EXPECT))
def test_oracle_decisions_keep_their_margin(programs, cid):
    case = K.solve_cases()[cid]
    prog = programs[case["prog"]]
    orc = K.case_oracle(prog, case)
    conv, *_ = orc.solve(case["x0"], case["guess"])
    steps = orc.step_indices()
    assert (orc.n_iter, bool(conv), max(steps), orc.clipped()) == EXPECT[cid]
    assert min(steps) >= 0                     # (no case ends on the failure test)
    m = orc.margins()
    assert min(m.values()) >= K.MARGIN, m


def test_case_shapes_are_what_they_are_chosen_for(programs):
    wide = programs["smooth_n(62,1)"]
    assert wide.system.obs_dim + wide.system.ctrl_dim == 63 and wide.jvp.n_slots == 136
    full = K.make_oracle(wide, 4)
    assert full.solve(K.solve_cases()["D-H4"]["x0"], np.zeros((4, 1)))[0] and full.n_iter == 21
    # ... and past the full LDS map: the sweep's workspace alone (its cost block of 62 observations: 7880 values); the
    # plan runs on the compact map, the sweep without its copy of the cost block
    cs = K.cost_block_stride(62, 1)
    assert 8 * K.ilqr_work_total(62, 1, cs) == 191408 > K.LDS_LIMIT and K.plan_lds_bytes(62, 1, wide.n_slots, cs) == 216240
    assert K.plan_compact_bytes(62, 1, wide.n_slots, cs) == (89240, 128368)
    fits = programs["smooth_n(53,1)"]            # case E: the widest smooth_n(n, 1) whose plan fits the full map
    assert K.plan_lds_bytes(53, 1, fits.n_slots, K.cost_block_stride(53, 1)) == 162144 <= K.LDS_LIMIT
    assert K.plan_lds_bytes(54, 1, fits.n_slots + 1, K.cost_block_stride(54, 1)) > K.LDS_LIMIT
    mid = programs["exact_n(17,6)"]
    assert mid.system.obs_dim > 16 and mid.system.obs_dim + mid.system.ctrl_dim == 23


def test_lds_map_of_the_refused_and_the_accepted_plan():
    """The arithmetic of the two-tier test (tests/test_gpu_program_ilqr.py): 45 states, 8 controls.  The rows
    [16][54], the next states [16][45] and s slots [s][16] take 864 + 720 + 16 s values, the workspace 15235 with its
    cost block of 4252: 8 * (16819 + 16 s) bytes <= 163840 up to s = 228."""
    cs = K.cost_block_stride(45, 8)
    assert cs == 2 * 45 * 45 + 64 + 3 * 45 + 2 + 1 == 4252
    assert K.ilqr_work_total(45, 8, cs) == 15235
    for s in (53, 228, 229, 256):
        assert K.plan_lds_bytes(45, 8, s, cs) == 8 * (864 + 720 + 16 * s + 15235)
    assert K.plan_lds_bytes(45, 8, 228, cs) <= K.LDS_LIMIT < K.plan_lds_bytes(45, 8, 229, cs)
    assert K.plan_compact_bytes(45, 8, 229, cs) == (80424, 87864)


def test_no_program_within_the_limits_is_over_the_compact_map():
    """Every nx + nu <= 63 (nu <= 16) at the 256 slots ampc_set_program allows: the compact line search and the sweep
    without the cost block stay inside a workgroup's LDS, so a plan's LDS refusal has no instance."""
    worst = [0, 0]
    for nu in range(1, 17):
        for nx in range(1, 64 - nu):
            a, b = K.plan_compact_bytes(nx, nu, 256, K.cost_block_stride(nx, nu))
            worst = [max(worst[0], a), max(worst[1], b)]
    assert worst == [113304, 128368] and max(worst) <= K.LDS_LIMIT
