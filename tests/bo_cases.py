"""The yardstick of the Bayesian-optimisation proposal (autompc_amd/tuning/proposer.py, steps 2-5) and the cases the
host and the GPU tests share.

A dense reference in plain loops and numpy, parametrised by dtype (``np.float64`` or ``np.longdouble``): an unblocked
Cholesky, row-by-row substitution, the greedy picks -- its own, or a REPLAY of a given pick sequence.  It imports
nothing from the code under test.

Tolerances are not fixed numbers.  For each of lml, mu, sigma^2 and EI a case's tolerance is
    100 x (largest difference between the float64 and the long-double run of this reference on that case)
    + FLOOR x max(1, largest magnitude of the quantity in the case),
The factor 100 is the margin ``sysid.lasso_fit.TIE`` takes over its measured form error, for the same reason: the
device sums in another order than any host code.  The floor, FLOOR = 2^-40, covers the cases in which the two
reference runs happen to agree to the last bit (n = 1, 2: a handful of operations) while the code under test forms
exp, erfc, log and the distance sum with other, equally legitimate roundings: a kernel value carries up to about
d eps ~ 1.4e-14 of such error at d = 64, and 2^-40 = 9.1e-13 leaves that a factor 64 for its way through the solve.
Cases that amplify more (small noise, long length scales) show it in the measured term.

Picks are checked by replay: the long-double reference follows the picks of the code under test; at every step the
reference EI of the pick must be within the EI tolerance of the reference's largest EI among the unpicked points, and
the reported pick_ei within tolerance of the reference's value.
"""
import functools
import math
from statistics import NormalDist

import numpy as np

VAR_FLOOR = 1e-12
FLOOR = 2.0 ** -40
LD = np.longdouble


# ---- special functions ---------------------------------------------------------------------------------------
def erfc(x, dtype):
    """erfc of an array.  float64: math.erfc.  long double: for |x| < 1.5 the series erf(x) = 2 / sqrt(pi) exp(-x^2)
    sum_k 2^k x^(2k+1) / (2k+1)!! (all terms positive), else the continued fraction exp(-x^2) / sqrt(pi) / (x +
    (1/2) / (x + 1 / (x + (3/2) / (x + ...)))) evaluated bottom-up from depth 200 (truncation below 1e-25 for
    x >= 1.5); erfc(-x) = 2 - erfc(x)."""
    x = np.asarray(x, dtype=dtype)
    if dtype is np.float64:
        return np.array([math.erfc(v) for v in x.ravel()], dtype=np.float64).reshape(x.shape)
    a = np.abs(x)
    out = np.empty_like(a)
    small = a < dtype(1.5)
    if np.any(small):
        xs = a[small]
        term, total = xs.copy(), xs.copy()
        for k in range(1, 400):
            term = term * (2 * xs * xs) / dtype(2 * k + 1)
            new = total + term
            if np.all(new == total):
                break
            total = new
        out[small] = 1 - 2 / np.sqrt(_pi(dtype)) * np.exp(-xs * xs) * total
    if np.any(~small):
        xb = a[~small]
        f = xb.copy()
        for k in range(200, 0, -1):
            f = xb + dtype(k) / 2 / f
        out[~small] = np.exp(-xb * xb) / np.sqrt(_pi(dtype)) / f
    return np.where(x < 0, 2 - out, out)


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def rank_transform(scores):
    """Step 2 in plain loops: non-finite scores count as +inf, average ranks for ties, z = Phi^-1((rank - 1/2) / n)."""
    s = [float(v) if math.isfinite(v) else math.inf for v in scores]
    n = len(s)
    z = []
    inv = NormalDist().inv_cdf
    for i in range(n):
        less = sum(1 for v in s if v < s[i])
        equal = sum(1 for v in s if v == s[i])
        rank = less + (equal + 1) / 2.0
        z.append(inv((rank - 0.5) / n))
    return np.array(z)


# ---- the reference -------------------------------------------------------------------------------------------
def kernel(A, B, w, dtype):
    """k(A, B): the squared distance summed over the dimensions in order."""
    s2 = np.zeros((A.shape[0], B.shape[0]), dtype=dtype)
    for k in range(A.shape[1]):
        t = (A[:, k, None] - B[None, :, k]) * w[k]
        s2 = s2 + t * t
    s = np.sqrt(dtype(5)) * np.sqrt(s2)
    return (1 + s + s * s / 3) * np.exp(-s)


def cholesky(K):
    """Unblocked, row by row; None when a pivot is not positive and finite."""
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        piv = K[j, j] - np.dot(L[j, :j], L[j, :j])
        if not (piv > 0 and np.isfinite(piv)):
            return None
        L[j, j] = np.sqrt(piv)
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def forward(L, B):
    """L^-1 B row by row (B [n] or [n][M])."""
    out = np.zeros_like(B)
    for i in range(L.shape[0]):
        out[i] = (B[i] - L[i, :i] @ out[:i]) / L[i, i]
    return out


def ei_of(mu, var, zmin, dtype):
    sd = np.sqrt(var)
    u = (zmin - mu) / sd
    Phi = erfc(-u / np.sqrt(dtype(2)), dtype) / 2
    phi = np.exp(-u * u / 2) / np.sqrt(2 * _pi(dtype))
    return sd * (u * Phi + phi)


class Fit:
    """Steps 3 and 4 of one case in one dtype."""

    def __init__(self, case, dtype):
        X, z, hw, hn, P = (np.asarray(case[k], dtype=dtype) for k in ("X", "z", "hyper_w", "hyper_noise", "pool"))
        self.dtype, self.P = dtype, P
        n, G = X.shape[0], hw.shape[0]
        self.lml = np.full(G, -np.inf, dtype=dtype)
        self.status = np.zeros(G, dtype=np.int32)
        self.chosen, best = -1, None
        for g in range(G):
            K = kernel(X, X, hw[g], dtype)
            K[np.diag_indices(n)] += hn[g]
            L = cholesky(K)
            if L is None:
                self.status[g] = 1
                continue
            t = forward(L, z)
            self.lml[g] = -np.dot(t, t) / 2 - np.sum(np.log(np.diag(L)))
            if self.chosen < 0 or self.lml[g] > self.lml[self.chosen]:
                self.chosen, best = g, (L, t)
        if self.chosen < 0:
            return
        self.use_row(self.chosen, X, z, hw, hn, best)

    def use_row(self, g, X, z, hw, hn, Lt=None):
        """The posterior of hyperparameter row g (the chosen one unless a test asks for another)."""
        dtype = self.dtype
        if Lt is None:
            K = kernel(X, X, hw[g], dtype)
            K[np.diag_indices(X.shape[0])] += hn[g]
            L = cholesky(K)
            Lt = (L, forward(L, z))
        L, t = Lt
        self.row, self.w, self.noise, self.zmin = g, hw[g], hn[g], np.min(z)
        self.V = forward(L, kernel(X, self.P, self.w, dtype))
        self.mu = self.V.T @ t
        self.var = np.maximum(1 - np.sum(self.V * self.V, axis=0), dtype(VAR_FLOOR))

    def replay(self, q, picks=None):
        """Step 5.  picks None: the reference's own greedy sequence; else the given one is followed.  Returns (picks,
        EI arrays [q][m] as they stood before each pick, the variances after the last update)."""
        dtype, m = self.dtype, self.P.shape[0]
        var, rows, taken, eis = self.var.copy(), [], [], []
        for step in range(q):
            ei = ei_of(self.mu, var, self.zmin, dtype)
            eis.append(ei)
            if picks is None:
                free = [i for i in range(m) if i not in taken]
                j = free[int(np.argmax(np.where(np.isnan(ei[free]), -np.inf, ei[free])))]
            else:
                j = int(picks[step])
            taken.append(j)
            c = kernel(self.P, self.P[j:j + 1], self.w, dtype)[:, 0] - self.V.T @ self.V[:, j]
            for r in rows:
                c = c - r * r[j]
            r = c / np.sqrt(max(c[j] + self.noise, dtype(VAR_FLOOR)))
            rows.append(r)
            var = np.maximum(var - r * r, dtype(VAR_FLOOR))
        return taken, np.array(eis), var


@functools.lru_cache(maxsize=None)
def _fits(name):
    case = CASES[name]
    return Fit(case, LD), Fit(case, np.float64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The long-double fit of a case, its own pick sequence and the case's tolerances {lml, mu, var, ei}: computed
    once per session, shared by every test, never modified."""
    case = CASES[name]
    ld, f64 = _fits(name)
    tol, worst = {}, {}
    if ld.chosen < 0:
        return ld, None, None, tol, worst
    ok = ld.status == 0
    assert np.array_equal(ld.status, f64.status)
    if f64.chosen != ld.chosen:                     # (two rows within the float64 error of each other)
        X, z, hw, hn = (np.asarray(case[k], dtype=np.float64) for k in ("X", "z", "hyper_w", "hyper_noise"))
        f64.use_row(ld.chosen, X, z, hw, hn)
    picks, eis, _ = ld.replay(case["q"])
    _, eis64, _ = f64.replay(case["q"], picks)

    def tolerance(key, a, b):
        a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
        worst[key] = float(np.max(np.abs(a - b)))
        tol[key] = 100.0 * worst[key] + FLOOR * max(1.0, float(np.max(np.abs(a))))

    tolerance("lml", ld.lml[ok], f64.lml[ok])
    tolerance("mu", ld.mu, f64.mu)
    tolerance("var", ld.var, f64.var)
    tolerance("ei", eis, eis64)
    return ld, picks, eis, tol, worst


def check_result(name, res, verbose=True):
    """A result dict of the code under test (``_lib.bo_propose`` / ``gp_propose_host``) against the reference of case
    `name`: statuses, chosen row, lml, mu, var by value, picks by replay."""
    case = CASES[name]
    ld, _, _, tol, worst = reference(name)
    assert np.array_equal(res["status"], ld.status), (name, res["status"], ld.status)
    if ld.chosen < 0:
        assert res["chosen"] == -1 and np.all(np.asarray(res["picks"]) == -1)
        return
    ok = ld.status == 0
    if verbose:
        print("%s: f64-vs-long-double lml %.2e mu %.2e var %.2e ei %.2e" % (name, worst["lml"], worst["mu"],
                                                                         worst["var"], worst["ei"]))
    err = np.abs(np.asarray(res["lml"], dtype=LD)[ok] - ld.lml[ok])
    assert np.all(np.isneginf(np.asarray(res["lml"])[~ok]))
    assert float(np.max(err)) <= tol["lml"], (name, "lml", float(np.max(err)), tol["lml"])
    # the chosen row: the reference's, unless another accepted row's lml is within tolerance of it
    ch = int(res["chosen"])
    assert ch >= 0 and ok[ch], (name, "chosen", ch)
    assert ch == ld.chosen or float(ld.lml[ld.chosen] - ld.lml[ch]) <= 2 * tol["lml"], (name, "chosen", ch, ld.chosen)
    if ch != ld.chosen:
        print("%s: rows %d and %d tie within the lml tolerance; posterior not compared" % (name, ch, ld.chosen))
        return
    errs = {"lml": float(np.max(err))}
    for key in ("mu", "var"):
        errs[key] = float(np.max(np.abs(np.asarray(res[key], dtype=LD) - getattr(ld, key))))
    if verbose:
        print("%s: under test lml %.2e (tol %.2e) mu %.2e (tol %.2e) var %.2e (tol %.2e); ei tol %.2e"
              % (name, errs["lml"], tol["lml"], errs["mu"], tol["mu"], errs["var"], tol["var"], tol["ei"]))
    for key in ("mu", "var"):
        assert errs[key] <= tol[key], (name, key, errs[key], tol[key])
    picks = [int(j) for j in res["picks"]]
    q = case["q"]
    assert len(picks) == q and len(set(picks)) == q and min(picks) >= 0 and max(picks) < case["pool"].shape[0]
    _, eis, _ = ld.replay(q, picks)
    for step, j in enumerate(picks):
        free = np.ones(eis.shape[1], dtype=bool)
        free[picks[:step]] = False
        top = float(np.max(eis[step][free]))
        assert top - float(eis[step][j]) <= tol["ei"], (name, "pick", step, j, top - float(eis[step][j]), tol["ei"])
        err = abs(float(res["pick_ei"][step]) - float(eis[step][j]))
        assert err <= tol["ei"], (name, "pick_ei", step, err, tol["ei"])
        others = free.copy()
        others[j] = False
        second = float(np.max(eis[step][others])) if others.any() else 0.0
        if top > 1e3 * tol["ei"]:                   # the margin is a ratio: checked where the ratio is well defined
            want = (float(eis[step][j]) - second) / float(eis[step][j])
            assert abs(float(res["pick_margin"][step]) - want) <= 4 * tol["ei"] / top, (name, "margin", step)


# ---- the cases -----------------------------------------------------------------------------------------------
def small_table(d, G=3):
    """G rows of moderate conditioning: isotropic length scales 0.2, 0.4, 0.8, ... with noise 1e-2, 1e-4, 1e-3, ..."""
    ls = [0.2, 0.4, 0.8, 0.3, 0.6, 1.2]
    ns = [1e-2, 1e-4, 1e-3]
    w = np.array([np.full(d, 1.0 / (ls[g % 6] * math.sqrt(d))) for g in range(G)])
    return w, np.array([ns[g % 3] for g in range(G)])


def default_table(d):
    """The proposer's default table, written out again here (tests/bo_cases.py imports nothing from it)."""
    ls, ns = (0.1, 0.2, 0.4, 0.8, 1.6, 3.2), (1e-6, 1e-4, 1e-2, 1e-1)
    return (np.array([np.full(d, 1.0 / (l * math.sqrt(d))) for l in ls for _ in ns]),
            np.array([s for _ in ls for s in ns]))


def ard_table(d, G, seed):
    """G rows with per-dimension length scales (ARD) and noise over 1e-5..1e-1."""
    rng = np.random.default_rng(seed)
    w = 1.0 / (10 ** rng.uniform(-0.7, 0.3, size=(G, d)) * math.sqrt(d))
    return w, 10 ** rng.uniform(-5, -1, size=G)


def make_case(n, d, m, q, seed, table=None, G=3, dup_x=False, ties=False, cluster=False):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    if dup_x and n >= 2:
        X[1] = X[0]                                  # (rows 0 and 1: the second pivot of a noise-0 row is exactly 0)
        if n >= 8:
            X[n - 1] = X[n // 2]
    # a closed-loop-cost-like score: a bowl in the exponent, a non-finite slab
    centre = np.linspace(0.3, 0.7, d)
    scores = 10 ** (3 * np.sum((X - centre) ** 2, axis=1) / max(1.0, d / 4) + 0.1 * rng.standard_normal(n))
    scores[X[:, 0] > 0.9] = np.inf
    if ties and n >= 4:
        scores[1::3] = scores[0]
    pool = rng.random((m, d))
    if cluster and m >= 8:
        pool[m // 2:m // 2 + 4] = pool[3]            # points snapped onto each other
    w, noise = table if table is not None else small_table(d, G)
    return dict(X=X, z=rank_transform(scores), hyper_w=w, hyper_noise=noise, pool=pool, q=q)


def _declined_cases():
    base = make_case(24, 5, 70, 8, 50, dup_x=True)
    w, noise = base["hyper_w"], base["hyper_noise"]
    with_row = dict(base, hyper_w=np.array([w[0], w[1], w[2]]), hyper_noise=np.array([noise[0], 0.0, noise[2]]))
    without = dict(base, hyper_w=np.array([w[0], w[2]]), hyper_noise=np.array([noise[0], noise[2]]))
    twins = dict(base, hyper_w=np.array([w[0], w[0], w[1]]), hyper_noise=np.array([noise[0], noise[0], noise[1]]))
    none = dict(base, hyper_w=np.array([w[0], w[1]]), hyper_noise=np.array([0.0, 0.0]))
    return {"declined_between": with_row, "declined_without": without, "twin_rows": twins, "all_declined": none}


CASES = {}
for _n in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100):
    CASES["n%d" % _n] = make_case(_n, 9, 70, 8, 100 + _n)
for _d in (1, 2, 64):
    CASES["d%d" % _d] = make_case(33, _d, 70, 8, 200 + _d)
for _m in (1, 63, 64, 65, 257):
    for _q in sorted({1, min(_m, 16)}):
        CASES["m%d_q%d" % (_m, _q)] = make_case(20, 5, _m, _q, 300 + _m)
CASES["m5_q5"] = make_case(20, 5, 5, 5, 310)
CASES["G1"] = make_case(40, 6, 70, 8, 400, G=1)
CASES["G24"] = make_case(40, 6, 70, 8, 401, table=default_table(6))
CASES["G64"] = make_case(40, 6, 70, 8, 402, table=ard_table(6, 64, 402))
CASES.update(_declined_cases())
CASES["dup_x"] = make_case(40, 6, 70, 8, 500, dup_x=True)
CASES["z_ties"] = make_case(40, 6, 70, 8, 501, ties=True)
CASES["pool_cluster"] = make_case(40, 6, 70, 8, 502, cluster=True)
SMALL_CASES = sorted(CASES)
# the multi-block paths: several panels, several pool blocks, the default table
CASES["mid"] = make_case(513, 13, 4096, 64, 600, table=default_table(13))
