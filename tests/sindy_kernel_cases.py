"""Shared by tests/test_sindy_kernels_host.py and tests/test_gpu_sindy_kernels.py: libraries that take the single-model
SINDy kernels (csrc/sindy_kernels.hpp) across every size their code branches on.

  tag    nx / nu  library                                        n_feat n_trig n_tab staged(f64)  what it reaches
  s5      5 / 1   trig 1 + interaction, continuous                  78     6    13   yes   lane-spread, first nx on the full-width
                                                                                          reduction; leftover feature loop at G 16 / 32
  s8      8 / 2   trig 2, poly 2, discrete                          60    20    51   yes   lane-spread at the last nx it takes; second
                                                                                          trig loop at G 16; no leftover at G 32 / 64
  s8w     8 / 6   trig 2, discrete                                  70    28    57   yes   nu 6 in the lane-spread body; leftover at G 32
  s6x     6 / 1   trig 1 + interaction, poly 3, cross terms,       217     7   127   yes   monomials and powers in the table, non-strict
                  continuous, strict_reference False                                       Jacobian of every kind; leftover at G 64
  s5p     5 / 1   poly 2, discrete                                  12     0     7   yes   fewer features than lanes (12 < 16): lanes
                                                                                          without a hoisted feature; no trig argument
  s7      7 / 1   trig 1, poly 2, continuous                        32     8    25   yes   exactly 2 x 16 features: G = 16 ends on the hoisted
  s7t     7 / 1   trig 3, poly 2, discrete                          64    24    57   yes   exactly 2 x 32 features; 24 trig arguments
  s8t     8 / 8   trig 3, poly 2, discrete                         128    48   113   yes   exactly 2 x 64 features; 48 trig arguments: three
                                                                                          rounds of the trig loop at G = 16; 8 controls
  s9      9 / 1   trig 1 + interaction, discrete                   210    10    21   yes   first nx on the LDS-accumulate branch: one thread
  t160   47 / 6   trig 1, poly 2, continuous                       212    53   160   no    the largest table in product form, unstaged
  t163   48 / 6   trig 1, poly 2, continuous                       216     0     0   no    one variable more: direct evaluation
  max    64 / 16  poly 2, discrete                                 160     0    81   no    the ABI's limits; 64 x 64 Jacobian per thread
  lds    30 / 8   trig 2, discrete                                 190    76   153   yes   a 48 048-byte staged program on wide columns:
                                                                                          forward kernel 161 216 B, MPPI unstaged
  m40    40 / 6   trig 1, poly 2, continuous                       184    46   139   no    t160's branch in an MPPI plan (see below)
  m56    56 / 16  poly 2, discrete                                 144     0    73   no    max's branch in an MPPI plan, 16 controls
  st_lo / st_hi   trig 1 + interaction, discrete, nu 1 (13 / 14 states)                   the pair found by staging_pair(): the largest
                                                                                          staged program (45 656 B) and the first that is
                                                                                          not (56 000 B)

Two cases a reader may look for and not find, both because of the code's own limits:
  * A 7 / 1 library with poly 3 and cross terms "with its monomials in the table": eight variables give 140 monomials,
    16 powers and 8 trig arguments, n_tab = 173 > 160 -- direct evaluation (t163's branch), not the table.  `s6x` is that
    library on one state fewer: n_tab = 127, in the table, still past four states.
  * f64 MPPI plans on `t160` and `max`: their one-thread rollout needs 170 080 B and 184 752 B of LDS -- the cost block of
    47 / 64 states alone is 36 / 68 KB -- and ampc_mppi_plan_create has always refused them.  The GPU test checks that
    refusal and runs the rollouts on `m40` and `m56`: the same libraries on fewer states, the largest that fit
    (142 240 B and 156 912 B), the same branches of the kernel (an unstaged product table of trig and power entries
    past eight states; a power-only table with 16 controls).  The model surface runs all four.

Coefficients: 0.9 I on the states for discrete libraries, a small stable block for continuous ones, and in EVERY feature
column one entry of magnitude in [0.01, 0.05] with a random sign in a random row -- so that a dropped, duplicated or
mis-indexed feature moves the result (tests/test_sindy_kernels_host.py checks that on the CPU).  Inputs are uniform in
[-0.8, 0.8].  Coefficients and inputs of a tag come from one seeded generator."""
import functools
import zlib

import numpy as np

from autompc_amd import SINDy
from autompc_amd.evaluation.model_metrics import sindy_program_sizes
from helpers import make_system

LDS_LIMIT = 160 * 1024                    # kLdsLimit (csrc/host_common.hpp)
STAGE_LIMIT = 48 * 1024                   # kSindyStageBytes (csrc/sindy_kernels.hpp)
ROWS = (1, 63, 64, 65, 130)
DT = 0.05


def _case(nx, nu, trig=0, inter=False, poly=1, cross=False, mode="discrete", strict=True):
    return dict(nx=nx, nu=nu, strict=strict,
                hyper=dict(trig_freq=trig, trig_interaction=inter, poly_degree=poly, poly_cross_terms=cross, time_mode=mode))


CASES = {
    "s5": _case(5, 1, 1, True, mode="continuous"),
    "s8": _case(8, 2, 2, poly=2),
    "s8w": _case(8, 6, 2),
    "s6x": _case(6, 1, 1, True, 3, True, "continuous", strict=False),
    "s5p": _case(5, 1, 0, poly=2),
    "s7": _case(7, 1, 1, poly=2, mode="continuous"),
    "s7t": _case(7, 1, 3, poly=2),
    "s8t": _case(8, 8, 3, poly=2),
    "s9": _case(9, 1, 1, True),
    "t160": _case(47, 6, 1, poly=2, mode="continuous"),
    "t163": _case(48, 6, 1, poly=2, mode="continuous"),
    "max": _case(64, 16, 0, poly=2),
    "lds": _case(30, 8, 2),
    "m40": _case(40, 6, 1, poly=2, mode="continuous"),
    "m56": _case(56, 16, 0, poly=2),
}
# tag -> (n_feat, n_trig, n_tab, staged in f64, LDS bytes of sindy_forward_kernel in f64)
EXPECT = {
    "s5": (78, 6, 13, True, None),
    "s8": (60, 20, 51, True, None),
    "s8w": (70, 28, 57, True, None),
    "s6x": (217, 7, 127, True, None),
    "s5p": (12, 0, 7, True, None),
    "s7": (32, 8, 25, True, None),
    "s7t": (64, 24, 57, True, None),
    "s8t": (128, 48, 113, True, None),
    "s9": (210, 10, 21, True, None),
    "t160": (212, 53, 160, False, 133120),
    "t163": (216, 0, 0, False, None),
    "max": (160, 0, 81, False, None),
    "lds": (190, 76, 153, True, 161216),
    "m40": (184, 46, 139, False, None),
    "m56": (144, 0, 73, False, None),
}
F32_TAGS = ("s5", "s8", "s9", "t160", "t163")
SPREAD_TAGS = ("s5", "s8", "s8w", "s6x", "s5p", "s7", "s7t", "s8t")            # lane-spread with AMPC_SINDY_FP unset
THREAD_TAGS = ("s9", "m40", "m56")                    # one thread per sample whatever the setting
MPPI_REFUSED = ("t160", "max")                        # f64 plans that do not fit 160 KB of LDS: refused at creation
# a lane-spread tag whose lane-spread map does not fit at this horizon cap (two noise / action rows of cap x nu per
# sample) while the one-thread map (one row per plan) does: the launcher's fall-back
FALLBACK = ("s8w", 1700)
# (nx, n_feat, n_trig, n_pow, n_mon, n_pool, n_tab) of a descriptor list that ampc_set_sindy takes and whose f64
# prediction is refused: 79 features sin(f v) of 79 distinct (variable, frequency) arguments on 64 states / 16 controls
RAW_PRED_REFUSED = (64, 79, 79, 0, 0, 0, 159)


def _constructor(hyper):
    return dict(trig_basis=hyper["trig_freq"] > 0, trig_freq=max(hyper["trig_freq"], 1),
                trig_interaction=hyper["trig_interaction"], poly_basis=hyper["poly_degree"] > 1,
                poly_degree=hyper["poly_degree"], poly_cross_terms=hyper["poly_cross_terms"], time_mode=hyper["time_mode"])


@functools.lru_cache(maxsize=None)
def staging_pair():
    """(nx below, nx above): trig 1 + interaction, discrete, one control -- the largest nx whose f64 program is staged
    (<= 48 KB) and the next one, found by computing sindy_prog_elems."""
    prev = None
    for nx in range(2, 64):
        c = _case(nx, 1, 1, True)
        m = SINDy(make_system(nx, 1, DT), **_constructor(c["hyper"]))
        staged = prog_bytes(sizes_of(m), 8) <= STAGE_LIMIT
        if prev is not None and prev[1] and not staged:
            return prev[0], nx
        prev = (nx, staged)
    raise AssertionError("no staging boundary below 64 states")


def case(tag):
    if tag in CASES:
        return CASES[tag]
    lo, hi = staging_pair()
    return _case({"st_lo": lo, "st_hi": hi}[tag], 1, 1, True)


ALL_TAGS = tuple(CASES) + ("st_lo", "st_hi")


def system(tag):
    c = case(tag)
    return make_system(c["nx"], c["nu"], DT)


def _seed(tag):
    return zlib.crc32(tag.encode())


@functools.lru_cache(maxsize=None)
def coefficients(tag):
    c = case(tag)
    nx, nu = c["nx"], c["nu"]
    nf = SINDy(system(tag), **_constructor(c["hyper"])).coefficients.shape[1]
    rng = np.random.default_rng(_seed(tag))
    Xi = np.zeros((nx, nf))
    if c["hyper"]["time_mode"] == "discrete":
        Xi[:, :nx] = 0.9 * np.eye(nx)
    else:
        Xi[:, :nx] = -0.5 * np.eye(nx) + 0.1 * rng.normal(size=(nx, nx)) / np.sqrt(nx)
    rows = rng.integers(nx, size=nf)
    Xi[rows, np.arange(nf)] += rng.uniform(0.01, 0.05, size=nf) * rng.choice([-1.0, 1.0], size=nf)
    Xi.setflags(write=False)
    return Xi


@functools.lru_cache(maxsize=None)
def inputs(tag, rows=130):
    c = case(tag)
    rng = np.random.default_rng(_seed(tag) + 1)
    s, u = rng.uniform(-0.8, 0.8, size=(rows, c["nx"])), rng.uniform(-0.8, 0.8, size=(rows, c["nu"]))
    s.setflags(write=False), u.setflags(write=False)
    return s, u


def model(tag, precision="f64", strict=None, Xi=None):
    c = case(tag)
    m = SINDy(system(tag), precision=precision, strict_reference=c["strict"] if strict is None else strict,
              **_constructor(c["hyper"]))
    m.set_coefficients(coefficients(tag) if Xi is None else Xi)
    return m


def oracle(tag, strict=None, Xi=None):
    from oracle.sindy import SINDyOracle
    c = case(tag)
    return SINDyOracle(system(tag), coefficients(tag) if Xi is None else Xi,
                       strict_reference=c["strict"] if strict is None else strict, **c["hyper"])


@functools.lru_cache(maxsize=None)
def s9_restriction():
    """(Xi9, keep, Xi8): s9's coefficients with rows 0..7 cut off from the ninth state (their entries on every feature
    that reads x8 are zero; row 8 reads everything), the mask of the features that do not read x8, and the 8-state model
    those rows are: the 8 / 1 library enumerates exactly the kept features, in the same order."""
    kind, a0, a1 = model("s9").library[:3]
    keep = ~((a0 == 8) | (a1 == 8))
    Xi9 = np.array(coefficients("s9"))
    Xi9[:8, ~keep] = 0.0
    rng = np.random.default_rng(_seed("s9") + 5)
    for k in np.nonzero(keep)[0]:
        if not np.any(Xi9[:8, k]):
            Xi9[k % 8, k] = rng.uniform(0.01, 0.05) * rng.choice([-1.0, 1.0])
    Xi9[8, Xi9[8] == 0.0] = 0.02
    Xi8 = Xi9[:8][:, keep].copy()
    assert Xi8.shape == SINDy(make_system(8, 1, DT), **_constructor(case("s9")["hyper"])).coefficients.shape
    for a in (Xi9, keep, Xi8):
        a.setflags(write=False)
    return Xi9, keep, Xi8


def s9_model8(precision="f64"):
    m = SINDy(make_system(8, 1, DT), precision=precision, **_constructor(case("s9")["hyper"]))
    m.set_coefficients(s9_restriction()[2])
    return m


def s9_oracle8():
    from oracle.sindy import SINDyOracle
    return SINDyOracle(make_system(8, 1, DT), s9_restriction()[2], **case("s9")["hyper"])


# ---- sizes: the formulas of csrc/sindy_kernels.hpp and csrc/mppi_sindy_choice_host.hpp, restated ---------------------
def sizes_of(m):
    """(nx, n_feat, n_trig, n_pow, n_mon, n_pool, n_tab) of a SINDy model's feature program."""
    return (m.system.obs_dim,) + tuple(sindy_program_sizes(m))


def sizes(tag):
    return sizes_of(model(tag))


def prog_bytes(sz, esz):
    """sindy_prog_elems x the element size."""
    nx, n_feat, n_trig, n_pow, n_mon, n_pool, _ = sz
    ints = 2 * n_feat + n_trig + n_pow + 2 * n_mon + 2 * n_pool
    return (n_feat * nx + n_trig + n_pow + (ints * 4 + esz - 1) // esz + 2) * esz


def stage_bytes(sz, esz):
    """sindy_stage_bytes: 0 when the program is not copied to LDS."""
    b = prog_bytes(sz, esz)
    return b + 2 * esz if sz[6] > 0 and b <= STAGE_LIMIT else 0


def forward_lds(sz, nu, esz):
    return (2 * sz[0] + nu + sz[6]) * 64 * esz + stage_bytes(sz, esz)


def cost_stride(no, nu):
    return (2 * no * no + nu * nu + 3 * no + 2 + 3) // 4 * 4


def thread_lds(sz, nu, esz, staged=True):
    return ((2 * sz[0] + nu + sz[6]) * 64 + cost_stride(sz[0], nu) + 3 * nu + 2) * esz + (stage_bytes(sz, esz) if staged else 0)


def spread_lds(sz, nu, esz, G, max_h):
    hcap = (max_h * nu + 3) // 4 * 4
    return ((64 // G) * (sz[0] + nu + sz[6] + 2 * hcap) + cost_stride(sz[0], nu) + 3 * nu + 2) * esz + stage_bytes(sz, esz)


def natural_lanes(num_path):
    samples = sum((int(n) + 63) // 64 * 64 for n in num_path)
    return 64 if samples <= 2048 else (32 if samples <= 8192 else 16)


# ---- MPPI plans ------------------------------------------------------------------------------------------------------
HORIZON_CAP = 8
PLANS = (((1, 2), (5, 8)), ((65, 8), (130, 2)))       # two plans of two problems (N, H) each
NATURAL = ((2100, 3, 32), (8200, 3, 16))              # (N, H, lanes the launcher picks by itself) on s5
SIGMA, LMDA = 0.04, 0.7
LO, HI = -0.6, 0.8
COSTS = ("diag", "dense", "indicator")


@functools.lru_cache(maxsize=None)
def plan_data(tag, problems=PLANS[0], cost="diag"):
    """Per problem N, H, x0, warm start [H][nu], noise [N][H][nu], Q / R / F (diagonal, or dense symmetric positive
    definite) and a goal.  Read-only."""
    c = case(tag)
    nx, nu = c["nx"], c["nu"]
    rng = np.random.default_rng(_seed(tag) + 2 + 17 * sum(n for n, _ in problems))
    B = len(problems)

    def block(n, lo, hi):
        d = np.diag(rng.uniform(lo, hi, n))
        if cost != "dense":
            return d
        W = rng.normal(size=(n, n))
        return d + 0.3 * lo * (W @ W.T) / n
    x0 = rng.uniform(-0.3, 0.3, size=(B, nx))
    x0[1::2, 0] = 0.32                                # every second problem starts beyond the indicator threshold on state 0
    d = dict(N=np.array([n for n, _ in problems], dtype=np.int32), H=np.array([h for _, h in problems], dtype=np.int32),
             x0=x0,
             act=[rng.normal(scale=0.4, size=(h, nu)) for _, h in problems],
             eps=[rng.normal(scale=np.sqrt(SIGMA), size=(n, h, nu)) for n, h in problems],
             Q=np.stack([block(nx, 0.5, 2.0) for _ in range(B)]), R=np.stack([block(nu, 0.01, 0.1) for _ in range(B)]),
             F=np.stack([block(nx, 0.5, 2.0) for _ in range(B)]), goal=rng.normal(scale=0.1, size=(B, nx)))
    for v in d.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return d


def indicator_limits(nx):
    """The terms of mppi_sindy_table_cases.indicator_terms for nx states: a threshold of 0.25 on states 0 and 1 about
    zero, and the box [-0.3, 0.35] with its first lower and last upper bound open."""
    limits = np.tile([-0.3, 0.35], (nx, 1))
    limits[0, 0], limits[nx - 1, 1] = -np.inf, np.inf
    return limits


def indicator_terms(tag):
    from autompc_amd import BoxThresholdCost, ThresholdCost
    from autompc_amd.costs.blocks import mppi_cost_parts
    s = system(tag)
    nx = s.obs_dim
    cost = ThresholdCost(s, np.zeros(nx), [0, 2], 0.25) + BoxThresholdCost(s, indicator_limits(nx))
    return mppi_cost_parts(cost, nx, s.ctrl_dim)[1]


@functools.lru_cache(maxsize=None)
def cpu_rollouts(tag, problems=PLANS[0], cost="diag"):
    """Every problem's costs [N], clipped noise [H][N][nu] and updated sequence [H][nu] from the oracle's MPPI on the
    oracle's SINDy model, fed the plan's warm start and noise."""
    from oracle.costs import BoxCostOracle, QuadCostOracle, SumCostOracle, ThresholdCostOracle
    from oracle.mppi import MPPIOracle
    c = case(tag)
    nx, nu = c["nx"], c["nu"]
    d = plan_data(tag, problems, cost)
    om = oracle(tag)
    out = []
    for b, (N, H) in enumerate(problems):
        oc = QuadCostOracle(d["Q"][b], d["R"][b], d["F"][b], d["goal"][b])
        if cost == "indicator":
            oc = SumCostOracle([oc, ThresholdCostOracle(np.zeros(nx), [0, 2], 0.25), BoxCostOracle(indicator_limits(nx))])
        np.random.seed(0)
        orc = MPPIOracle(om, oc, np.tile([LO, HI], (nu, 1)), horizon=H, num_path=N, sigma=SIGMA, lmda=LMDA)
        orc.act_sequence = np.array(d["act"][b])
        costs, eps = orc.do_rollouts(np.array(d["x0"][b]), np.array(d["eps"][b]))
        orc.update(costs, eps)
        out.append((costs, eps, orc.act_sequence.copy()))
    return out


# ---- iLQR problems ---------------------------------------------------------------------------------------------------
ILQR_TAGS = ("s5", "s9")
ILQR_H = (1, 5)
ILQR_BOUNDS = (-0.4, 0.6)


@functools.lru_cache(maxsize=None)
def ilqr_problem(tag):
    c = case(tag)
    nx, nu = c["nx"], c["nu"]
    rng = np.random.default_rng(_seed(tag) + 3)
    return dict(Q=np.eye(nx), R=0.1 * np.eye(nu), F=5.0 * np.eye(nx), x0=rng.uniform(-0.3, 0.3, size=nx))


@functools.lru_cache(maxsize=None)
def ilqr_oracle(tag, H, perturbed=False):
    """The oracle's iLQR with bounded controls; perturbed: on coefficients (1 + 1e-12 standard normal), elementwise."""
    from oracle.costs import QuadCostOracle
    from oracle.ilqr import ILQROracle
    c = case(tag)
    nx, nu = c["nx"], c["nu"]
    p = ilqr_problem(tag)
    Xi = np.array(coefficients(tag))
    if perturbed:
        Xi = Xi * (1.0 + 1e-12 * np.random.default_rng(_seed(tag) + 4).normal(size=Xi.shape))
    orc = ILQROracle(oracle(tag, strict=True, Xi=Xi), QuadCostOracle(p["Q"], p["R"], p["F"], np.zeros(nx)), DT, H,
                     ubounds=(np.full(nu, ILQR_BOUNDS[0]), np.full(nu, ILQR_BOUNDS[1])))
    conv, st, ct, Ks, ks = orc.solve(np.array(p["x0"]), np.zeros((H, nu)))
    return dict(converged=bool(conv), iters=int(orc.n_iter), states=st, ctrls=ct, Ks=Ks)
