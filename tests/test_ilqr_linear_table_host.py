"""The host side of the iLQR plan that holds a table of linear models of mixed state dimension (no GPU):
``ilqr_linear_table_decision``, the evaluator's constructor argument, the tuner's model sub-space, the bindings, the
packer's offsets and strides against a numpy restatement, and the precondition of the GPU tests' decision checks --
the oracle's iLQR takes the same decisions on every problem of tests/ilqr_linear_table_cases.py whether it runs on
(A, B) or on (A, B) perturbed by 1e-12 relative."""
import numpy as np
import pytest

import ilqr_linear_table_cases as C
from autompc_amd import ARX, MLP, Koopman, SINDy, System
from autompc_amd.tuning.batch_eval import ilqr_linear_table_decision
from helpers import rel_err


def _system(nu=2):
    return System(["x0", "x1", "x2"], ["u%d" % i for i in range(nu)], dt=0.05)


def _cand(model=None):
    c = dict(horizon=5, Q=np.ones(3), R=np.ones(2), F=np.ones(3))
    if model is not None:
        c["model"] = model
    return c


def _arx(s, history, **kw):
    m = ARX(s, history=history, **kw)
    rng = np.random.default_rng(history)
    m.set_parameters({"coeffs": 0.1 * rng.normal(size=(s.obs_dim, m._get_fvec_size()))})
    return m


def _koop(s, **kw):
    m = Koopman(s, **kw)
    n = m.state_dim
    m.set_parameters({"A": 0.5 * np.eye(n), "B": 0.1 * np.ones((n, s.ctrl_dim))})
    return m


def test_ilqr_linear_table_decision():
    s = _system()
    own = _arx(s, 2)
    a, b = _arx(s, 1), _arx(s, 10)
    k = _koop(s, poly_basis="true", poly_degree=3, trig_basis="true", trig_freq=2)
    ident = _koop(s)
    assert ilqr_linear_table_decision([_cand(a), _cand(k), _cand(), _cand(b), _cand(ident)], own) == (True, "")
    assert ilqr_linear_table_decision([_cand(), _cand()], own, "f64", 0, 3, 2) == (True, "")
    # linear_table_decision's verdicts carry over
    mlp = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    ok, why = ilqr_linear_table_decision([_cand(a), _cand(mlp)], own)
    assert not ok and "MLP is not an ARX or Koopman model" in why
    ok, why = ilqr_linear_table_decision([_cand(a), _cand(SINDy(s))], own)
    assert not ok and "SINDy is not an ARX or Koopman model" in why
    assert ilqr_linear_table_decision([_cand(a), _cand(k)], mlp) == (True, "")    # (nobody runs on the evaluator's own)
    ok, why = ilqr_linear_table_decision([_cand(a), _cand(ARX(s, history=3))], own)
    assert not ok and "not trained" in why
    ok, why = ilqr_linear_table_decision([_cand(_koop(s, poly_basis="true", poly_degree=2, product_terms="true"))], own)
    assert not ok and "product terms" in why
    ok, why = ilqr_linear_table_decision([_cand(_arx(s, 2, device=1))], own)
    assert not ok and "device" in why
    # f64 only
    ok, why = ilqr_linear_table_decision([_cand(_arx(s, 2, precision="f32"))], _arx(s, 3, precision="f32"), precision="f32")
    assert not ok and "f64 only" in why
    # at most 128 states: an ARX of history 26 has 1 + 26 * 3 + 25 * 2 = 129, of history 25 it has 124
    assert _arx(s, 25).state_dim == 124 and _arx(s, 26).state_dim == 129
    assert ilqr_linear_table_decision([_cand(_arx(s, 25))], own) == (True, "")
    ok, why = ilqr_linear_table_decision([_cand(a), _cand(_arx(s, 26))], own)
    assert not ok and "129 states, more than 128" in why
    # the sweep's control dimensions
    for nu, fine in ((1, True), (4, True), (5, False), (6, True), (7, False), (8, True)):
        sn = _system(nu)
        m = _arx(sn, 2)
        ok, why = ilqr_linear_table_decision([dict(_cand(m), R=np.ones(nu))], m)
        assert ok == fine and (fine or "1, 2, 3, 4, 6 or 8 controls" in why)
    # an observation dimension no plan handle can be staged with (an identity network up to 63 - nu, wide above 64)
    s62 = System(["x%d" % i for i in range(62)], ["u0", "u1"], dt=0.05)
    m62 = _koop(s62)
    ok, why = ilqr_linear_table_decision([_cand(m62)], m62)
    assert not ok and "no plan handle" in why


def _task(s):
    from autompc_amd import QuadCost, Task
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(3), np.eye(2), np.eye(3)))
    task.set_ctrl_bounds(-np.ones(2), np.ones(2))
    task.set_init_obs(np.zeros(3))
    task.set_num_steps(5)
    return task


def test_evaluator_checks_its_argument():
    from autompc_amd.tuning import IlqrCandidateEvaluator
    s = _system()
    task = _task(s)
    own = _arx(s, 2)
    assert IlqrCandidateEvaluator(s, task, own).linear_models == "shape"
    assert IlqrCandidateEvaluator(s, task, own, linear_models="table").linear_models == "table"
    for bad in ("single", "Table", None, 1):
        with pytest.raises(ValueError, match="linear_models"):
            IlqrCandidateEvaluator(s, task, own, linear_models=bad)
    with pytest.raises(ValueError, match="one_plan=True"):
        IlqrCandidateEvaluator(s, task, own, linear_models="table", one_plan=False)
    # a Koopman model, or an ARX with a surrogate that is not itself: refused by default, taken under "table"
    mlp = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    k = _koop(s, poly_basis="true", poly_degree=3)
    for model, sur in ((own, mlp), (k, None), (k, mlp)):
        with pytest.raises(TypeError, match="candidates with simulate\\(\\) and the drop-in controller"):
            IlqrCandidateEvaluator(s, task, model, surrogate=sur)
        ev = IlqrCandidateEvaluator(s, task, model, surrogate=sur, linear_models="table")
        # ... and a batch that does not take the table gets the constructor's refusal from evaluate()
        with pytest.raises(TypeError, match="candidates with simulate\\(\\) and the drop-in controller"):
            ev.evaluate([_cand(), _cand(mlp)], n_steps=2)


def test_tuner_draws_linear_model_configurations_for_a_table_evaluator():
    from autompc_amd.sysid.linear import ARXFactory, KoopmanFactory
    from autompc_amd.tuning import BatchPipelineTuner, IlqrCandidateEvaluator
    s = _system()
    task = _task(s)
    mlp = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    ev = IlqrCandidateEvaluator(s, task, _arx(s, 2), surrogate=mlp, linear_models="table")
    tuner = BatchPipelineTuner(s, ev, model_factory=ARXFactory(s), trajs=[])
    cands = tuner.ask(12, np.random.default_rng(0))
    assert all(set(c["model_cfg"]) == {"history"} and 1 <= c["model_cfg"]["history"] <= 10 for c in cands)
    assert len({c["model_cfg"]["history"] for c in cands}) > 1
    assert all("sigma" not in c and 5 <= c["horizon"] <= 25 for c in cands)        # (iLQR candidates)
    tuner = BatchPipelineTuner(s, ev, model_factory=KoopmanFactory(s), trajs=[])
    cands = tuner.ask(12, np.random.default_rng(0))
    assert all("method" in c["model_cfg"] and "poly_basis" in c["model_cfg"] for c in cands)
    # the default evaluator keeps what the tuner did before
    ev0 = IlqrCandidateEvaluator(s, task, mlp)
    tuner = BatchPipelineTuner(s, ev0, model_factory=ARXFactory(s), trajs=[])
    assert all("history" not in c["model_cfg"] for c in tuner.ask(4, np.random.default_rng(0)))


def test_prototypes_of_the_new_entries():
    from ctypes import POINTER, c_double, c_int, c_longlong, c_void_p
    from autompc_amd import _lib
    ip, dp = POINTER(c_int), POINTER(c_double)
    assert _lib.SIGNATURES["ampc_ilqr_plan_set_linear_models"] == (c_int, [c_void_p, c_int, POINTER(c_void_p), ip, ip, ip, dp])
    ll = POINTER(c_longlong)
    assert _lib.SIGNATURES["ampc_ilqr_linear_table_layout"] == (c_int, [c_int, ip, c_int, c_int, c_int, c_int, c_int, ll, ll])
    assert _lib.SIGNATURES["ampc_ilqr_closed_loop_linear"] == (
        c_int, [c_void_p, c_void_p, c_int, dp, dp, ip, ip, ip, c_int, c_int, dp, dp, ip, ip, POINTER(c_longlong)])
    assert hasattr(_lib.IlqrPlan, "set_linear_models") and hasattr(_lib.IlqrPlan, "closed_loop_linear")
    lib = _lib.load()                                   # (the library exports them)
    assert lib.ampc_ilqr_plan_set_linear_models and lib.ampc_ilqr_closed_loop_linear


# ---- the packer's layout, restated ---------------------------------------------------------------------------------------
def _up(a, m):
    return (a + m - 1) // m * m


def pack_entry(A, B):
    """One table entry as ampc_ilqr_plan_set_linear_models packs it: the MFMA fragments of M = [A | B] in
    set_linear_wide's order wf[tile][k-step][lane] = M[16 tile + (lane & 15)][4 k-step + (lane >> 4)], the plain rows
    (padded to a multiple of four values), the sweep's zero-padded Jacobian jp [nxp][ldj]."""
    nx, nu = B.shape
    k, nxp, kp, ldj = nx + nu, _up(nx, 16), _up(nx + nu, 4), _up(nx + nu, 16)
    M = np.zeros((nxp, max(kp, ldj)))
    M[:nx, :k] = np.hstack([A, B])
    lane = np.arange(64)
    wf = np.stack([np.stack([M[16 * nt + (lane & 15), 4 * ks + (lane >> 4)] for ks in range(kp // 4)])
                   for nt in range(nxp // 16)])
    plain = np.zeros(_up(nx * k, 4))
    plain[:nx * k] = np.hstack([A, B]).ravel()
    return dict(wf=wf.ravel(), plain=plain, jp=M[:, :ldj].ravel(), nxp=nxp, kp=kp, ldj=ldj, ntile=nxp // 16, ksn=kp // 4)


def table_layout(nxs, nu, B, H, ls_n=10):
    """Offsets (in values) of every entry's three parts in the table buffer, and the strides of the per-slot regions:
    those of the plan's horizon and of the WIDEST entry."""
    off, o = [], 0
    for nx in nxs:
        k, nxp = nx + nu, _up(nx, 16)
        wf, plain, jp = (nxp // 16) * (_up(k, 4) // 4) * 64, _up(nx * k, 4), nxp * _up(k, 16)
        off.append((o, o + wf, o + wf + plain))
        o += wf + plain + jp
    w = max(nxs)
    strides = dict(states=(H + 1) * w, ctrls=H * nu, Ks=H * nu * w, ks=H * nu, ls_states=ls_n * (H + 1) * w,
                   ls_ctrls=ls_n * H * nu, vj=_up(w, 16) * _up(w + nu, 16))
    return off, o, strides


def lds_bytes(nx, nu, no):
    """LDS of the sweep (make_wide_lds) and of the line search ([x | u] rows at an odd stride, next states, the compact
    work map with the cost block) for the widest entry, in bytes."""
    nsp, n, nu4 = _up(nx, 16), nx + nu, _up(nu, 4)
    sweep = nsp * (nsp + 1) + nsp + _up(n, 4) + 3 * nu4 * (nsp + 1) + nu4 * nu4 + 3 * no + nsp + nu4 + 8
    cs = _up(2 * no * no + nu * nu + 3 * no + 2, 4)
    xs = _up(n, 4) | 1
    work = _up(_up(16 * xs, 4) + 16 * nx, 4)
    wk = nu * nx + nu + nu + nu * nu + nx + nu + cs + nu + nu + 16 + 16 + (nu + 1) // 2 + 8
    return _up(sweep, 4) * 8, (work + wk) * 8


def test_the_lds_refusal_is_where_the_gpu_test_puts_it():
    """90 observations, 2 controls: a 90-state table fits 160 KB, a 128-state entry's line search does not."""
    from autompc_amd import _lib
    fits = _lib.ilqr_linear_table_layout([90], 2, 90, 1, 2)[1]
    wide = _lib.ilqr_linear_table_layout([90, 128], 2, 90, 1, 2)[1]
    assert (fits["sweep_lds_bytes"], fits["ls_lds_bytes"]) == lds_bytes(90, 2, 90)
    assert (wide["sweep_lds_bytes"], wide["ls_lds_bytes"]) == lds_bytes(128, 2, 90)
    assert max(fits["sweep_lds_bytes"], fits["ls_lds_bytes"]) <= 160 * 1024 < wide["ls_lds_bytes"]
    assert wide["sweep_lds_bytes"] <= 160 * 1024


@pytest.mark.parametrize("name", sorted(C.SETS))
def test_the_packers_offsets_and_strides(name):
    system, ab = C.matrices(name)
    s = C.SETS[name]
    nu = s["nu"]
    off, total, strides = table_layout(s["nx"], nu, 4, C.PLAN_H)
    w = max(s["nx"])
    assert strides["states"] == (C.PLAN_H + 1) * w and strides["vj"] % 256 == 0
    # the library's own numbers (ampc_ilqr_linear_table_layout, which ampc_ilqr_plan_set_linear_models packs by)
    from autompc_amd import _lib
    lib_off, lib = _lib.ilqr_linear_table_layout(s["nx"], nu, s["no"], 4, C.PLAN_H, 10)
    assert [tuple(int(v) for v in row) for row in lib_off] == off and lib["table_values"] == total
    assert {k: lib[k] for k in strides} == strides
    sweep, ls = lds_bytes(w, nu, s["no"])
    assert (lib["sweep_lds_bytes"], lib["ls_lds_bytes"]) == (sweep, ls) and max(sweep, ls) <= 160 * 1024
    o = 0
    for (A, B), (o_wf, o_plain, o_jp), nx in zip(ab, off, s["nx"]):
        e = pack_entry(A, B)
        assert (o_wf, o_plain, o_jp) == (o, o + e["wf"].size, o + e["wf"].size + e["plain"].size)
        o += e["wf"].size + e["plain"].size + e["jp"].size
        # a fragment holds its 16 x 4 block of M: tile nt, k-step ks, lane l -> M[16 nt + l % 16][4 ks + l // 16]
        M = np.hstack([A, B])
        wf = e["wf"].reshape(e["ntile"], e["ksn"], 64)
        for nt, ks, l in ((0, 0, 0), (e["ntile"] - 1, e["ksn"] - 1, 63), (e["ntile"] // 2, e["ksn"] // 2, 37)):
            r, c = 16 * nt + (l & 15), 4 * ks + (l >> 4)
            assert wf[nt, ks, l] == (M[r, c] if r < nx and c < nx + nu else 0.0)
        jp = e["jp"].reshape(e["nxp"], e["ldj"])
        np.testing.assert_array_equal(jp[:nx, :nx + nu], M)
        assert not np.any(jp[nx:]) and not np.any(jp[:, nx + nu:])
        # a problem's rows, packed at its own nx, fit the region of the widest entry
        assert (C.PLAN_H + 1) * nx <= strides["states"] and e["nxp"] * e["ldj"] <= strides["vj"]
    assert o == total
    # the boundaries the sets name
    if name == "edges":
        assert [(_up(n, 16), _up(n + nu, 16)) for n in s["nx"][:5]] == [(16, 16), (16, 16), (16, 32), (16, 32), (32, 32)]
    if name == "wide":
        assert s["nx"][:5] == (62, 64, 65, 126, 128) and 126 + nu == 128
    if name == "nu6":
        assert 122 + nu == 128


@pytest.mark.parametrize("name", sorted(C.SETS))
def test_the_cases_are_what_the_gpu_tests_assume(name):
    s = C.SETS[name]
    d = C.problems(name)
    P = len(d["index"])
    assert 4 < P <= 12 and max(s["hz"]) == C.PLAN_H and set(s["hz"]) == {1, 2, 5, 8}
    assert set(d["index"].tolist()) == set(range(len(s["nx"]) - 1))      # every model but the spare is used
    assert not np.all(np.diff(d["index"]) >= 0)                          # non-monotonic
    if name != "wide":
        assert s["nx"][0] == s["no"]                                     # rule 0's shape: the state is the observation
    assert all(x.shape == (s["nx"][k],) for x, k in zip(d["x0"], d["index"]))
    assert len({a.tobytes() for a in d["Q"]}) == P                       # per-problem cost blocks


@pytest.mark.parametrize("name", sorted(C.SETS))
def test_the_oracles_decisions_survive_a_perturbation_of_the_models(name):
    """The precondition of comparing the device's converged / iters with the oracle's: 1e-12 relative on (A, B) -- far
    more than the device's rounding differs from numpy's -- changes no decision and moves the states by less than the
    GPU test's bound."""
    plain, pert = C.oracle_solves(name), C.oracle_solves(name, True)
    clipped = 0
    for j, (a, b) in enumerate(zip(plain, pert)):
        assert (a["converged"], a["iters"]) == (b["converged"], b["iters"]), (name, j)
        assert rel_err(a["states"], b["states"]) < 1e-7 and rel_err(a["ctrls"], b["ctrls"]) < 1e-6, (name, j)
        assert rel_err(a["Ks"], b["Ks"]) < 1e-6
        assert a["iters"] < C.MAX_ITER
        clipped += int(np.sum(np.abs(a["ctrls"]) == 1.0))
    assert clipped > 0                                                   # the bounds bite somewhere
    assert len({a["iters"] for a in plain}) > 1                          # slots finish at different times
