"""What makes the rule of mlpfit_cases.py safe before a GPU sees it (the cases of test_gpu_mlpfit_edges.py; no GPU
here): the long-double reference against torch's own fit and against a committed golden of the reference project, the
conditions every case must meet (``d64 <= 1e-13``, no relu / selu hidden unit within 1e-9 of its kink), the teeth of
every case (a float64 restatement with a deliberate error departs by at least ten bounds), and the coverage the GPU file
claims.  Every figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

import mlpfit_cases as C
from autompc_amd.sysid import mlp_fit as F
from test_gpu_mlp_fit_device import SWEEP
from test_mlp_fit import TOL, _case

ALL = [c.name for c in C.CASES]


# ---- the reference itself -------------------------------------------------------------------------------------------
def _torch_orders(train_seed, n_rows, epochs):
    gen = F.seeded_generator(train_seed)
    return np.stack([F.epoch_order(gen, n_rows).numpy() for _ in range(epochs)])


def _against_torch(dims, act, feed, target, n_batch, lr, epochs, seed, train_seed):
    """(departure of fit_reference_style from the long-double reference, d64, bound) of one configuration."""
    ws, bs = F.initial_parameters(seed, dims)
    w0, b0 = [w.numpy() for w in ws], [b.numpy() for b in bs]
    orders = _torch_orders(train_seed, feed.shape[0], epochs)
    args = (dims, act, w0, b0, feed, target, orders, n_batch, lr)
    ref = C.flat(*C.fit_steps_ref(*args, np.longdouble)[:2])
    d64 = max(C.departure(C.flat(*C.fit_steps_ref(*args, np.float64, kernel_forms=True, reverse_rows=rev)[:2]), ref)
              for rev in (False, True))
    rw, rb = F.fit_reference_style(dims, act, torch.from_numpy(feed), torch.from_numpy(target), epochs, n_batch, lr,
                                   seed, train_seed=train_seed)
    d = C.departure(C.flat([w.numpy() for w in rw], [b.numpy() for b in rb]), ref)
    return d, d64, C.bound_of(d64)


SWEEP_PICK = [0, 1, 2, 3, 7, 11, 16]           # relu, tanh, sigmoid (lr 1e-5), selu (depth 3), selu (depth 4), tanh, sigmoid


def test_the_picked_sweep_shapes_cover_the_four_activations():
    assert {SWEEP[k][1] for k in SWEEP_PICK} == set(F.ACTS) and len(SWEEP_PICK) >= 4


@pytest.mark.parametrize("k", SWEEP_PICK)
def test_the_long_double_reference_agrees_with_torchs_fit_on_sweep_shapes(k):
    dims, act, nb, rows, lr, epochs = SWEEP[k]
    rng = np.random.default_rng(100 + k)                                   # the sweep's own data and seeds
    feed, target = rng.normal(size=(rows, dims[0])), rng.normal(size=(rows, dims[-1]))
    d, d64, bound = _against_torch(dims, act, feed, target, nb, lr, epochs, 40 + k, 7 + k)
    print("sweep %2d %-22s %-7s nb %3d rows %3d lr %g: torch vs long double %.3e, d64 %.3e, bound %.3e"
          % (k, dims, act, nb, rows, lr, d, d64, bound))
    assert d <= bound


def test_the_long_double_reference_reproduces_a_golden_of_the_reference_project():
    g, system, trajs, hidden, init, final = _case("hc_relu3")
    dims = [system.obs_dim + system.ctrl_dim] + hidden + [system.obs_dim]
    XU, dY, xm, xs, dm, ds = F.training_arrays(trajs)
    feed, target = F.normalised(XU, dY, xm, xs, dm, ds)
    n_iter, n_batch = int(g["n_train_iters"]), int(g["n_batch"])
    orders = _torch_orders(100, feed.shape[0], n_iter)                     # MLP.train's default train seed
    ws, bs, _ = C.fit_steps_ref(dims, str(g["activation"]), init[0::2], init[1::2], feed, target, orders, n_batch,
                                float(g["lr"]), np.longdouble)
    d = C.departure(np.concatenate([np.asarray(f).ravel() for f in final]), C.flat(ws, bs))   # weight, bias, weight ...
    print("golden hc_relu3 %s, %d steps: trained net vs long double %.3e (tolerance %.0e)"
          % (dims, n_iter * -(-feed.shape[0] // n_batch), d, TOL))
    assert d <= TOL


def test_clamping_and_the_two_forms_of_the_reference():
    np.testing.assert_array_equal(C.clamp_orders([-5, -1, 0, 3, 4, 9, 2 ** 31 - 1], 4), [0, 0, 0, 3, 3, 3, 3])
    z = np.array([-1.5, -1e-3, 0.0, 1e-3, 2.0], dtype=np.longdouble)
    for act in C.ACTS:                       # derivative from the result == from the pre-activation, to rounding
        a, b = C._deriv_from_result(act, C._act(act, z)), C._deriv_from_z(act, z)
        assert float(np.max(np.abs(a - b))) < 1e-18, act
    assert float(C._deriv_from_z("relu", z)[2]) == 0.0                               # at z == 0: torch's convention
    assert float(C._deriv_from_z("selu", z)[2]) == float(np.longdouble(C.SELU_SCALE) * np.longdouble(C.SELU_ALPHA))
    assert np.all(np.diff(C._act("selu", z)) > 0)
    h = np.longdouble(2) ** -20                                                      # a central difference of act
    for act in C.ACTS:
        x = np.array([-0.7, 0.4], dtype=np.longdouble)
        fd = (C._act(act, x + h) - C._act(act, x - h)) / (2 * h)
        assert float(np.max(np.abs(fd - C._deriv_from_z(act, x)))) < 1e-11, act


# ---- conditions on every case the GPU file uses ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_every_case_is_well_conditioned(name):
    c, r = C.BY_NAME[name], C.reference(name)
    steps = c.epochs * -(-c.n_rows // c.n_batch)
    print("%-18s %-20s %-7s nb %4d rows %4d lr %g, %2d steps: d64 %.3e, bound %.3e, smallest hidden |z| %.3e"
          % (name, c.dims, c.act, c.n_batch, c.n_rows, c.lr, steps, r.d64, r.bound, min(r.min_z)))
    assert len(r.min_z) == steps
    assert r.d64 <= C.D64_MAX and r.bound <= 1e-11
    assert min(r.min_z) >= C.Z_MIN
    assert c.lr in (3e-3, 1e-2)
    moved = C.departure(r.f64, C.flat(*C.initial(name)))
    assert moved > 0.5 * c.lr                                     # Adam's first steps move a parameter by about lr


@pytest.mark.parametrize("name", ALL)
def test_every_case_has_teeth(name):
    c, r = C.BY_NAME[name], C.reference(name)
    ragged = c.n_rows % c.n_batch != 0
    for change in C.TEETH:
        if change == "full_batch_divisor" and not ragged:
            continue
        moved = C.departure(C.flat(*C.run(name, np.float64, kernel_forms=True, change=change)[:2]), r.f64)
        print("%-18s %-18s moves the parameters by %.3e = %.1e bounds" % (name, change, moved, moved / r.bound))
        assert moved >= 10.0 * r.bound, change


def test_the_exact_zero_cases_have_exact_zeros():
    for name in C.names("zero"):
        c = C.BY_NAME[name]
        trace = []
        C.run(name, np.longdouble, trace=trace)
        z = trace[0]["z"][0]
        n0 = int(np.sum(z == 0))
        print("%s: %d of %d hidden pre-activations are exactly 0" % (name, n0, z.size))
        assert len(trace) == 1 and n0 == C.exact_zero_count(name) >= C.ZERO_FORCED
        # every forward sum is exact in float64: float64 and long double give the same pre-activations, all dyadic
        t64 = []
        C.run(name, np.float64, kernel_forms=True, trace=t64)
        z64 = t64[0]["z"][0]
        np.testing.assert_array_equal(z64.astype(np.longdouble), z)
        np.testing.assert_array_equal(z64 * 32, np.rint(z64 * 32))
        # the convention is visible: taking the other side of the kink at the zeros moves the parameters
        ws, bs = C.initial(name)
        feed, target = C.data(name)
        nudged = [bs[0] + 2.0 ** -40] + list(bs[1:])
        p = C.flat(*C.fit_steps_ref(list(c.dims), c.act, ws, nudged, feed, target, C.orders(name), c.n_batch, c.lr,
                                    np.float64, kernel_forms=True)[:2])
        moved = C.departure(p - C.flat(ws, nudged) + C.flat(ws, bs), C.reference(name).f64)
        print("%s: z = +2^-40 instead of 0 moves the parameters by %.3e" % (name, moved))
        assert moved >= 10.0 * C.reference(name).bound


# ---- coverage -------------------------------------------------------------------------------------------------------
def test_the_cases_cover_what_the_gpu_file_claims():
    by = {g: [C.BY_NAME[n] for n in C.names(g)] for g in ("batch", "wide", "pair", "order", "mixed", "zero", "forty")}
    assert sum(len(v) for v in by.values()) == len(C.CASES) and len(set(ALL)) == len(ALL)
    steps = lambda c: c.epochs * -(-c.n_rows // c.n_batch)
    # batch rows past 128: one full step then one row; and one plan whose only batch is ragged
    full = [c for c in by["batch"] if c.n_rows == c.n_batch + 1]
    assert [c.n_batch for c in full] == [129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096]
    assert all(c.dims == (7, 33, 5) and steps(c) == 2 for c in full)
    assert any(c.n_batch == 4096 and c.n_rows == 100 for c in by["batch"])
    assert {c.act for c in by["batch"]} == set(C.ACTS) and max(c.n_batch for c in C.CASES) == F.DEVICE_MAX_BATCH
    # wide layers on a long batch
    assert {(c.dims, c.act, c.n_batch, c.n_rows) for c in by["wide"]} == {
        ((80, 256, 256, 64), "relu", 257, 300), ((80, 255, 17, 64), "selu", 129, 130)}
    # phase A's row-tile pairs: 2, 3, 3, 4 row tiles in the first step
    assert [(c.n_batch, c.n_rows) for c in by["pair"]] == [(32, 63), (33, 65), (48, 95), (49, 97)]
    assert all(c.dims == (6, 65, 17, 3) for c in by["pair"])
    assert sorted({-(-c.n_batch // 16) for c in by["pair"]}) == [2, 3, 4]
    # row orders
    assert [c.order for c in by["order"]] == ["identity", "repeat", "outside", "clamped"]
    assert all((c.dims, c.n_batch, c.n_rows) == ((5, 33, 16, 3), 17, 40) for c in by["order"])
    rep, out, cl = (C.orders("order_" + k)[0] for k in ("repeat", "outside", "clamped"))
    first = list(rep[:17])
    assert max(first.count(v) for v in first) == 3 and len(set(range(40)) - set(rep)) >= 1
    assert {-1, 40, 45, 2 ** 31 - 1} <= set(out.tolist()) and out.min() < 0 and out.max() > 39
    np.testing.assert_array_equal(cl, C.clamp_orders(out, 40))
    assert cl.min() >= 0 and cl.max() <= 39 and not np.array_equal(cl, out)
    same = by["order"][2]._replace(name="", order="")                      # one fit, but for the order as uploaded
    assert same == by["order"][3]._replace(name="", order="")
    np.testing.assert_array_equal(C.reference("order_outside").params, C.reference("order_clamped").params)
    for nm in ("order_repeat", "order_outside"):                           # ... and not the identity order's fit
        c = C.BY_NAME[nm]
        plain = C.flat(*C.fit_steps_ref(list(c.dims), c.act, *C.initial(nm), *C.data(nm), C.orders("order_identity"),
                                        c.n_batch, c.lr, np.float64, kernel_forms=True)[:2])
        assert C.departure(plain, C.reference(nm).f64) > 1e-6
    # mixed plan, free layout
    assert [len(c.dims) - 2 for c in by["mixed"]] == [1, 4, 2, 1, 3]
    assert {c.act for c in by["mixed"]} == set(C.ACTS) and {c.lr for c in by["mixed"]} == {3e-3, 1e-2}
    assert len({(c.dims[0], c.dims[-1], c.n_batch, c.n_rows, c.epochs) for c in by["mixed"]}) == 1
    assert by["mixed"][0].epochs == 2
    offs, total, canary = C.mixed_layout()
    spans = sorted((int(o), int(o) + C.n_params(c.dims)) for o, c in zip(offs, by["mixed"]))
    assert any(offs[j] < offs[i] for i in range(5) for j in range(i + 1, 5))             # non-monotonic
    gaps = [b[0] - a[1] for a, b in zip(spans, spans[1:])]
    assert sorted(g for g in gaps if g) == [1, 7, 64] and min(gaps) >= 0 and spans[0][0] == 0
    assert total - spans[-1][1] == 64
    owned = np.zeros(total, dtype=int)
    for a, b in spans:
        owned[a:b] += 1
    owned[canary] += 1
    np.testing.assert_array_equal(owned, 1)
    assert len(canary) == 1 + 7 + 64 + 64
    # exact zeros, forty steps
    assert {c.act for c in by["zero"]} == {"relu", "selu"} and all(steps(c) == 1 for c in by["zero"])
    (f,) = by["forty"]
    assert (f.dims, f.act, f.n_batch, f.n_rows, f.epochs) == ((4, 17, 2), "tanh", 16, 32, 20)
    assert steps(f) == 40 and sum(C.FORTY_GROUPS) == 20 and C.FORTY_GROUPS == (7, 6, 7)
    assert all(steps(c) <= 3 for c in C.CASES if c.group not in ("mixed", "forty"))
    assert all(c.lr in (3e-3, 1e-2) for c in C.CASES)
