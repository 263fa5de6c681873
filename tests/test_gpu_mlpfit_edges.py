"""The MLP fit kernels (csrc/mlpfit_kernels.hpp, ampc_mlpfit_*) at their code's own edges, against the long-double
reference of mlpfit_cases.py: mini-batches of 129..4096 rows (phase B's 64-row chunks, the forward grid's row tiles),
fewer rows than n_batch, wide layers on a long batch, phase A's row-tile pairs (2, 3, 4 row tiles), row orders with
repeats and entries outside the data, a mixed-depth plan in a free parameter layout with canaries around every span,
hidden pre-activations of exactly 0, and forty steps of bias correction over three run_epoch groups.  ``-m gpu``.

The plan is driven directly (``_lib.MlpFitPlan``) with explicit int32 row orders.  One rule, fixed in mlpfit_cases.py and
made safe on the host by test_mlpfit_reference_host.py: the largest absolute parameter departure from the long-double
run is at most ``max(1e-13, 100 * d64)``.  Every comparison prints its figures before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import mlpfit_cases as C
from autompc_amd import _lib
from autompc_amd.sysid import mlp_fit as F

pytestmark = pytest.mark.gpu


def _fit(case_names, offsets=None, n_total=None, groups=None):
    """Train the cases `case_names` (one data set, one n_batch) in ONE plan; `offsets` / `n_total`: a free layout whose
    every double outside the models' spans holds the canary; `groups`: epochs per run_epoch group.  Returns (the flat
    buffer as float64 numpy, offsets, plan.steps)."""
    cs = [C.BY_NAME[n] for n in case_names]
    c0 = cs[0]
    assert all((c.n_batch, c.n_rows, c.epochs, C.data_seed(c)) == (c0.n_batch, c0.n_rows, c0.epochs, C.data_seed(c0))
               for c in cs)
    lay = F.pack_device_models([list(c.dims) for c in cs])
    if offsets is None:
        offsets, n_total = lay["offsets"], lay["n_params"]
    host = np.full(n_total, C.CANARY)
    for c, o in zip(cs, offsets):
        p = C.flat(*C.initial(c.name))
        host[o:o + p.size] = p
    feed, target = C.data(c0.name)
    dev = torch.device("cuda", torch.cuda.current_device())
    dfeed, dtarget, dflat = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (feed, target, host)]
    order = np.stack([C.orders(c.name) for c in cs], axis=1)                    # [epochs][K][n_rows], as uploaded
    assert order.min() >= -2 ** 31 and order.max() <= 2 ** 31 - 1
    didx = [torch.from_numpy(np.ascontiguousarray(o.astype(np.int32))).to(dev) for o in order]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev)
    plan = _lib.MlpFitPlan(lay["n_hidden"], lay["dims"], [c.act for c in cs], [c.lr for c in cs], offsets,
                           dfeed.data_ptr(), dtarget.data_ptr(), c0.n_rows, c0.n_batch, dflat.data_ptr(), n_total,
                           device=dev.index, stream=stream.cuda_stream)
    e = 0
    for n in groups or (c0.epochs,):
        for _ in range(n):
            plan.run_epoch(didx[e].data_ptr())
            e += 1
        stream.synchronize()
    assert e == c0.epochs
    steps = plan.steps
    out = dflat.cpu().numpy()
    plan.close()
    return out, np.asarray(offsets), steps


@functools.lru_cache(maxsize=None)
def _alone(name):
    """The case's device fit in a plan of one (flat parameters), computed once."""
    c = C.BY_NAME[name]
    out, _, steps = _fit([name])
    assert steps == c.epochs * -(-c.n_rows // c.n_batch) and out.size == C.n_params(c.dims)
    out.setflags(write=False)
    return out


def _hold(name, params, what=""):
    c, r = C.BY_NAME[name], C.reference(name)
    d = C.departure(params, r.params)
    moved = C.departure(params, C.flat(*C.initial(name)))
    print("%-18s %-20s %-7s nb %4d rows %4d lr %g%s: departure %.3e, d64 %.3e, bound %.3e (parameters moved %.3e)"
          % (name, c.dims, c.act, c.n_batch, c.n_rows, c.lr, what, d, r.d64, r.bound, moved))
    assert np.all(np.isfinite(params))
    assert moved > 0.5 * c.lr
    assert d <= r.bound


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names("batch"))
def test_batches_of_129_to_4096_rows(name):
    """n_rows = n_batch + 1: one full step, then a step of one row; and n_batch 4096 over 100 rows, where the only
    batch is ragged."""
    _hold(name, _alone(name))


@pytest.mark.parametrize("name", C.names("wide"))
def test_wide_layers_on_a_long_batch(name):
    _hold(name, _alone(name))


@pytest.mark.parametrize("name", C.names("pair"))
def test_row_tile_pairs_of_phase_a(name):
    """[6, 65, 17, 3] at n_batch 32, 33, 48, 49 over 2 n_batch - 1 rows: 2, 3, 3, 4 row tiles, then 2, 2, 3, 3."""
    _hold(name, _alone(name))


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names("order"))
def test_row_orders_with_repeats_and_entries_outside_the_data(name):
    _hold(name, _alone(name))


def test_an_order_outside_the_data_is_its_clamped_order_bit_for_bit():
    assert not np.array_equal(C.orders("order_outside"), C.orders("order_clamped"))
    np.testing.assert_array_equal(_alone("order_outside"), _alone("order_clamped"))
    assert not np.array_equal(_alone("order_outside"), _alone("order_identity"))


# 3 -------------------------------------------------------------------------------------------------------------------
def test_a_mixed_plan_in_a_free_layout_keeps_inside_its_spans():
    """Depths 1, 4, 2, 1, 3 in one plan; spans out of order in the buffer, gaps of 1, 7, 64 doubles and a 64-double
    tail, all holding a canary."""
    mixed = C.names("mixed")
    offsets, n_total, canary = C.mixed_layout()
    out, _, steps = _fit(mixed, offsets, n_total)
    assert steps == 6
    bits = out[canary].view(np.int64)
    assert np.array_equal(bits, np.full(len(canary), C.CANARY).view(np.int64))          # every canary bit-unchanged
    for name, o in zip(mixed, offsets):
        mine = out[o:o + C.n_params(C.BY_NAME[name].dims)]
        _hold(name, mine, " (in the plan of five)")
        np.testing.assert_array_equal(mine, _alone(name))                                # a neighbour changes nothing


# 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names("zero"))
def test_hidden_pre_activations_of_exactly_zero(name):
    """Dyadic data: every forward sum is exact, at least nine hidden pre-activations are exactly 0 (counted in the host
    test); the derivative there is 0 for relu and scale * alpha for selu."""
    assert C.exact_zero_count(name) >= C.ZERO_FORCED
    _hold(name, _alone(name))


# 5 -------------------------------------------------------------------------------------------------------------------
def test_forty_steps_of_bias_correction_over_three_groups():
    (name,) = C.names("forty")
    out, _, steps = _fit([name], groups=C.FORTY_GROUPS)
    assert steps == 40
    _hold(name, out, " (40 steps as 7 + 6 + 7 epochs)")
