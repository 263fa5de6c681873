"""The reference and the cases of the MLP fit kernels' edge tests (csrc/mlpfit_kernels.hpp, ampc_mlpfit_*), shared by
test_mlpfit_reference_host.py (CPU) and test_gpu_mlpfit_edges.py (MI355X).  Plain numpy.

``fit_steps_ref`` restates the reference's training loop (autompc/sysid/mlp.py:177-217: gathered mini-batch,
``act(A W' + b)``, SmoothL1Loss(beta = 1, mean), backward, torch's Adam with its defaults) on EXPLICIT row orders in any
numpy float type.  In ``np.longdouble`` it is written independently of the kernel (derivatives from the pre-activation,
textbook Adam); in float64 with ``kernel_forms=True`` it uses the expressions the kernel header documents.

The rule every comparison with the device uses, fixed here and not tuned on the device:

    bound = max(1e-13, 100 * d64)

``d64``: the larger absolute parameter departure from the long-double run of two float64 runs -- the kernel's forms, and
the same with every batch's rows taken in reversed order (another order of the sums over the batch).  100 x and the
1e-13 floor are the fits' rule (test_gpu_sindy_fit.py).
"""
import collections
import functools

import numpy as np

ACTS = ("relu", "tanh", "sigmoid", "selu")
B1, B2, EPS = 0.9, 0.999, 1e-8                                       # torch.optim.Adam's defaults
SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
FLOOR, FACTOR = 1e-13, 100.0
D64_MAX = 1e-13                                                      # a case's d64 may not exceed this: no bound > 1e-11
Z_MIN = 1e-9                                                         # no relu / selu hidden unit with 0 < |z| < Z_MIN
TEETH = ("grad_scale", "drop_last_row", "zero_bias_grad", "full_batch_divisor")


def clamp_orders(orders, n_rows):
    """Row-order entries as the library uses them: below 0 -> 0, at or past n_rows -> n_rows - 1 (ABI text)."""
    return np.clip(np.asarray(orders, dtype=np.int64), 0, n_rows - 1)


def _act(name, z):
    T = z.dtype.type
    if name == "relu":
        return np.where(z > 0, z, T(0))
    if name == "tanh":
        return np.tanh(z)
    if name == "sigmoid":
        return T(1) / (T(1) + np.exp(-z))
    return T(SELU_SCALE) * np.where(z > 0, z, T(SELU_ALPHA) * np.expm1(np.minimum(z, T(0))))


def _deriv_from_z(name, z):
    """act'(z) from the PRE-activation; at z == 0: relu 0, selu scale * alpha (torch's convention)."""
    T = z.dtype.type
    if name == "relu":
        return np.where(z > 0, T(1), T(0))
    if name == "tanh":
        t = np.tanh(z)
        return T(1) - t * t
    if name == "sigmoid":
        s = T(1) / (T(1) + np.exp(-z))
        return s * (T(1) - s)
    return np.where(z > 0, T(SELU_SCALE), T(SELU_SCALE) * T(SELU_ALPHA) * np.exp(np.minimum(z, T(0))))


def _deriv_from_result(name, a):
    """act' from the activation's RESULT, as mlpfit_kernels.hpp documents (fit_act_deriv)."""
    T = a.dtype.type
    if name == "relu":
        return np.where(a > 0, T(1), T(0))
    if name == "tanh":
        return T(1) - a * a
    if name == "sigmoid":
        return a * (T(1) - a)
    return np.where(a > 0, T(SELU_SCALE), a + T(SELU_SCALE) * T(SELU_ALPHA))


def fit_steps_ref(dims, act, W0, b0, feed, target, orders, n_batch, lr, dtype, kernel_forms=False, reverse_rows=False,
                  change=None, trace=None):
    """Train layer widths `dims` from (W0, b0) over `orders` [epochs][n_rows], every operation in `dtype`.

    Returns (weights, biases, min_z): the parameters as `dtype` arrays and, per optimiser step, the smallest |z| over
    the hidden relu / selu pre-activations that are not exactly zero (inf where there is none).
    `reverse_rows`: every batch's rows in reversed order (the sums over the batch take another order).
    `change`: one of TEETH, a deliberate error (grad_scale: every gradient x (1 + 1e-4); drop_last_row: the batch's
    last row left out of the weight gradients; zero_bias_grad; full_batch_divisor: the loss over n_batch * out).
    `trace`: a list that receives, per step, {"z": [...], "a": [...], "g": [...], "gW": [...], "gb": [...]}."""
    T = np.dtype(dtype).type
    L = len(dims) - 1
    W = [np.asarray(w, dtype=dtype).copy() for w in W0]
    b = [np.asarray(v, dtype=dtype).copy() for v in b0]
    feed, target = np.asarray(feed, dtype=dtype), np.asarray(target, dtype=dtype)
    n_rows = feed.shape[0]
    orders = clamp_orders(orders, n_rows)
    P = W + b
    M = [np.zeros_like(p) for p in P]
    V = [np.zeros_like(p) for p in P]
    b1, b2, eps, lr = T(B1), T(B2), T(EPS), T(lr)
    t, min_z = 0, []
    for order in orders:
        for s in range(0, n_rows, n_batch):
            idx = order[s:s + n_batch]
            if reverse_rows:
                idx = idx[::-1]
            nb = len(idx)
            A, Z = [feed[idx]], []
            for l in range(L):
                z = A[l] @ W[l].T + b[l]
                Z.append(z)
                A.append(_act(act, z) if l < L - 1 else z)
            mz = np.inf
            if act in ("relu", "selu"):
                for z in Z[:-1]:
                    az = np.abs(z[z != 0])
                    if az.size:
                        mz = min(mz, float(az.min()))
            min_z.append(mz)
            d = Z[-1] - target[idx]
            div = (n_batch if change == "full_batch_divisor" else nb) * dims[-1]
            g = np.where(np.abs(d) < 1, d, np.sign(d)) / T(div)
            gW, gb, G = [None] * L, [None] * L, [None] * L
            for l in range(L - 1, -1, -1):
                G[l] = g
                gw = g.copy()
                if change == "drop_last_row":
                    gw[0 if reverse_rows else -1] = 0
                gW[l] = gw.T @ A[l]
                gb[l] = np.zeros_like(b[l]) if change == "zero_bias_grad" else g.sum(axis=0)
                if l > 0:
                    g = (g @ W[l]) * (_deriv_from_result(act, A[l]) if kernel_forms else _deriv_from_z(act, Z[l - 1]))
            if trace is not None:
                trace.append({"z": Z, "a": A, "g": G, "gW": gW, "gb": gb})
            t += 1
            bc1, bc2 = T(1) - b1 ** t, T(1) - b2 ** t
            for k, gk in enumerate(gW + gb):
                if change == "grad_scale":
                    gk = gk * T(1 + 1e-4)
                if kernel_forms:                     # fit_adam: torch's _single_tensor_adam
                    M[k] = M[k] + (gk - M[k]) * (T(1) - b1)
                    V[k] = V[k] * b2 + (T(1) - b2) * gk * gk
                    P[k] -= (lr / bc1) * (M[k] / (np.sqrt(V[k]) / np.sqrt(bc2) + eps))
                else:                                # Kingma & Ba, algorithm 1
                    M[k] = b1 * M[k] + (T(1) - b1) * gk
                    V[k] = b2 * V[k] + (T(1) - b2) * gk * gk
                    P[k] -= lr * (M[k] / bc1) / (np.sqrt(V[k] / bc2) + eps)
    return P[:L], P[L:], min_z


def flat(ws, bs):
    """Weights and biases in the flat layout of one model: per layer the weight [out][in] row-major, then the bias."""
    return np.concatenate([np.concatenate([np.asarray(w).ravel(), np.asarray(v).ravel()]) for w, v in zip(ws, bs)])


def departure(ours, ref):
    """Largest absolute departure of flat parameters `ours` (float64) from `ref` (any type), taken in ref's type."""
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(ours).astype(ref.dtype) - ref)))


# ---- the cases ------------------------------------------------------------------------------------------------------
# order: "perm" (a permutation per epoch), "identity", "repeat" (a row three times in the first batch, another absent),
# "outside" (entries -1, n_rows, n_rows + 5, 2**31 - 1), "clamped" ("outside" already clamped), "exact" (identity; the
# dyadic data of the exact-zero cases).
Case = collections.namedtuple("Case", "name group dims act n_batch n_rows lr epochs seed order")


def _cases():
    out = []
    for i, nb in enumerate([129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096]):      # one full step, then one row
        out.append(Case("batch%d" % nb, "batch", (7, 33, 5), ACTS[i % 4], nb, nb + 1, (1e-2, 3e-3)[i % 2], 1, 300 + i,
                        "perm"))
    out.append(Case("batch4096_rows100", "batch", (7, 33, 5), "tanh", 4096, 100, 1e-2, 2, 310, "perm"))
    out.append(Case("wide_relu", "wide", (80, 256, 256, 64), "relu", 257, 300, 1e-2, 1, 320, "perm"))
    out.append(Case("wide_selu", "wide", (80, 255, 17, 64), "selu", 129, 130, 3e-3, 1, 321, "perm"))
    for i, nb in enumerate([32, 33, 48, 49]):                                         # row tiles 2, 3, 3, 4 then 2, 2, 3, 3
        out.append(Case("pair%d" % nb, "pair", (6, 65, 17, 3), ACTS[(i + 1) % 4], nb, 2 * nb - 1, (3e-3, 1e-2)[i % 2], 1,
                        330 + i, "perm"))
    for i, kind in enumerate(["identity", "repeat", "outside", "clamped"]):
        out.append(Case("order_" + kind, "order", (5, 33, 16, 3), ("relu", "tanh", "selu", "selu")[i], 17, 40, 1e-2, 1,
                        340, kind))                    # "outside" and "clamped" are one fit: bit-equal on the device
    for i, (hidden, act, lr) in enumerate([((17,), "relu", 1e-2), ((32, 31, 17, 63), "selu", 3e-3),
                                           ((64, 15), "tanh", 1e-2), ((33,), "sigmoid", 3e-3),
                                           ((16, 65, 33), "relu", 1e-2)]):                # depths 1, 4, 2, 1, 3
        out.append(Case("mixed%d" % i, "mixed", (5,) + hidden + (3,), act, 17, 40, lr, 2, 350 + i, "perm"))
    out.append(Case("zero_relu", "zero", (4, 17, 3), "relu", 19, 19, 1e-2, 1, 360, "exact"))
    out.append(Case("zero_selu", "zero", (4, 17, 3), "selu", 19, 19, 1e-2, 1, 361, "exact"))
    out.append(Case("forty", "forty", (4, 17, 2), "tanh", 16, 32, 3e-3, 20, 370, "perm"))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
FORTY_GROUPS = (7, 6, 7)                              # the forty steps' epochs, as three run_epoch groups on one plan
MIXED_GAPS, MIXED_TAIL, CANARY = (1, 7, 64), 64, -7.0e300
# The mixed plan's models in PLAN order are mixed0..mixed4; their spans lie in the flat buffer in this order:
MIXED_BUFFER_ORDER = (3, 0, 4, 1, 2)


def names(group):
    return [c.name for c in CASES if c.group == group]


def data_seed(case):
    """The cases of the order and mixed groups share one data set each (one plan, or one comparison across orders)."""
    return {"order": 340, "mixed": 350}.get(case.group, case.seed)


@functools.lru_cache(maxsize=None)
def data(name):
    """(feed [n_rows][in], target [n_rows][out]) float64."""
    c = BY_NAME[name]
    rng = np.random.default_rng(data_seed(c))
    if c.order == "exact":                            # multiples of 1/4 in [-2, 2]
        return rng.integers(-8, 9, size=(c.n_rows, c.dims[0])) / 4.0, rng.integers(-8, 9, size=(c.n_rows, c.dims[-1])) / 4.0
    feed = rng.normal(size=(c.n_rows, c.dims[0]))
    target = 0.5 * rng.normal(size=(c.n_rows, c.dims[-1])) + 0.25 * feed[:, :1]
    return feed, target


ZERO_FORCED = 9                                       # hidden units of an exact-zero case built to be 0 on one row


@functools.lru_cache(maxsize=None)
def initial(name):
    """(weights, biases) float64: F.initial_parameters' float32 draws; the exact-zero cases' are dyadic."""
    c = BY_NAME[name]
    if c.order == "exact":
        rng = np.random.default_rng(c.seed + 1000)
        feed, _ = data(name)
        ws = [rng.integers(-8, 9, size=(o, i)) / 8.0 for i, o in zip(c.dims[:-1], c.dims[1:])]
        bs = [rng.integers(-8, 9, size=o) / 8.0 for o in c.dims[1:]]
        for j in range(ZERO_FORCED):                  # unit j's pre-activation on row j: exactly 0 (multiples of 1/32)
            bs[0][j] = -(feed[j] @ ws[0][j])
        return ws, bs
    from autompc_amd.sysid import mlp_fit as F
    ws, bs = F.initial_parameters(c.seed, list(c.dims))
    return [w.numpy().copy() for w in ws], [v.numpy().copy() for v in bs]


@functools.lru_cache(maxsize=None)
def orders(name):
    """[epochs][n_rows] int64, as uploaded (NOT clamped)."""
    c = BY_NAME[name]
    n = c.n_rows
    if c.order in ("identity", "exact"):
        return np.tile(np.arange(n, dtype=np.int64), (c.epochs, 1))
    if c.order == "perm":
        rng = np.random.default_rng(7000 + data_seed(c))
        return np.stack([rng.permutation(n) for _ in range(c.epochs)]).astype(np.int64)
    o = np.tile(np.arange(n, dtype=np.int64), (c.epochs, 1))
    if c.order == "repeat":
        o[:, 3] = o[:, 9] = 5                         # row 5 three times in the first batch; rows 3 and 9 absent
        return o
    o[:, [0, 4, 16, 17, 39]] = [-1, n, n + 5, 2 ** 31 - 1, -2 ** 31]      # both batches of 17 and the ragged one
    return clamp_orders(o, n) if c.order == "clamped" else o


def exact_zero_count(name):
    """Hidden pre-activations of an exact-zero case's only step that are exactly 0, in integer arithmetic."""
    c = BY_NAME[name]
    (w0, *_), (b0, *_) = initial(name)
    feed, _ = data(name)
    z32 = np.rint(feed * 4).astype(np.int64) @ np.rint(w0 * 8).astype(np.int64).T + np.rint(b0 * 32).astype(np.int64)
    assert c.epochs == 1 and c.n_batch >= c.n_rows
    return int(np.sum(z32 == 0))


def run(name, dtype, **kw):
    c = BY_NAME[name]
    w0, b0 = initial(name)
    feed, target = data(name)
    return fit_steps_ref(list(c.dims), c.act, w0, b0, feed, target, orders(name), c.n_batch, c.lr, dtype, **kw)


Reference = collections.namedtuple("Reference", "params d64 bound min_z f64")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's long-double parameters (flat), d64, its bound, the per-step smallest |z|, the float64 kernel-form
    parameters (flat)."""
    ws, bs, min_z = run(name, np.longdouble)
    ref = flat(ws, bs)
    f64 = flat(*run(name, np.float64, kernel_forms=True)[:2])
    rev = flat(*run(name, np.float64, kernel_forms=True, reverse_rows=True)[:2])
    d64 = max(departure(f64, ref), departure(rev, ref))
    ref.setflags(write=False)
    f64.setflags(write=False)
    return Reference(ref, d64, max(FLOOR, FACTOR * d64), tuple(min_z), f64)


def bound_of(d64):
    return max(FLOOR, FACTOR * d64)


def n_params(dims):
    return sum(o * i + o for i, o in zip(dims[:-1], dims[1:]))


def mixed_layout():
    """The mixed plan's free layout: (param_offsets in PLAN order, n_params of the buffer, canary index array).  The
    spans lie in MIXED_BUFFER_ORDER with gaps of 1, 7, 64 and 0 doubles between them and a 64-double tail."""
    cs = [BY_NAME[n] for n in names("mixed")]
    gaps = list(MIXED_GAPS) + [0]
    offsets, canary, o = [0] * len(cs), [], 0
    for pos, k in enumerate(MIXED_BUFFER_ORDER):
        offsets[k] = o
        o += n_params(cs[k].dims)
        gap = gaps[pos] if pos < len(cs) - 1 else MIXED_TAIL
        canary += list(range(o, o + gap))
        o += gap
    return np.array(offsets, dtype=np.int64), o, np.array(canary, dtype=np.int64)
