"""Case tables of tests/test_gpu_lane_groups.py, plain data and helpers.  Test infrastructure only, no GPU code.

The small-matrix kernels of the non-parametric estimator -- ols_kernel / als_kernel / standardize_kernel (csrc/als.hip),
var_boot_kernel / quantile_kernel (csrc/boot.hip), chow_kernel (csrc/breaks.hip) -- share one shape: a group of R lanes owns
one problem, NG = 256 / R groups share a workgroup, and R is chosen from the regressor count by the switch of the kernel's
launch_* function.  That dispatch is restated here (the C++ stays the authority; tests/test_lane_group_cases_cpu.py pins the
restatement to the numbers the sources state), together with, per kernel, the cases the GPU tests run, the deterministic
generators of their inputs, and their CPU references in two formulations:

  "oracle"  as the project's oracles compute it: als_oracle._ols (LAPACK least squares), boot_oracle.var_bootstrap_irf,
            break_oracle.compute_chow;
  "other"   the same statistic with the solver exchanged: the normal equations where the oracle calls least squares (OLS and
            the VAR of every bootstrap draw -- the route the kernels take), and least squares (a pseudo-inverse) where the
            oracle solves normal equations (the HAC sandwich of the Chow statistic).

The CPU test asserts that the two agree to 1e-11 of the largest entry (1e-10 relative for the Chow statistic): the cases are
conditioned well enough that the 1e-9 / 1e-8 tolerances of the GPU tests cannot hide a wrong kernel behind the solver.
Every reference is computed once per process (functools.lru_cache) and must not be modified by its users.

Unless a case says otherwise it has 2 NG + 3 problems: three workgroups, the last one partial."""
import contextlib
import functools

import numpy as np

from oracle import als_oracle as ao
from oracle import boot_oracle as bo
from oracle import break_oracle as bk

THREADS = 256                        # kAlsThreads, kBootThreads, kChowThreads
LDS_LIMIT = 160 * 1024               # the refusal `lds > 160 * 1024` of launch_boot_r, launch_als_r, launch_quantiles


# ------------------------------------------------------------------------------------------------ dispatch restated
def pow2_ge(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def pad_r(n):
    """capi.hip pad_r: the power of two >= n, at least 2."""
    return max(2, pow2_ge(n))


def ols_width(K):
    """dfm_ols_batch_dev: launch_ols(K > 32 ? 64 : pad_r(K)); K > 64 is DFM_E_R_UNSUPPORTED (None)."""
    return None if K > 64 else (64 if K > 32 else pad_r(K))


def als_width(r):
    """dfm_als_batch_dev: launch_als(pad_r(r)); r > DFM_MAX_R = 32 is refused (None)."""
    return None if r > 32 else pad_r(r)


def boot_width(ns, p):
    """launch_var_boot: K = 1 + ns p regressors, R = 8, 16, 32 or 64; ns > 8 or K > 64 is refused (None)."""
    K = 1 + ns * p
    if ns > 8 or K > 64:
        return None
    return 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64


def chow_width(k):
    """launch_chow: 2 k regressors (levels and interactions), R = 2, 4, 8 or 16; k > 8 is refused (None)."""
    return None if k > 8 else (2 if k <= 1 else 4 if k <= 2 else 8 if k <= 4 else 16)


OLS_WIDTHS = (2, 4, 8, 16, 32, 64)
ALS_WIDTHS = (2, 4, 8, 16, 32)
BOOT_WIDTHS = (8, 16, 32, 64)
CHOW_WIDTHS = (2, 4, 8, 16)
# the largest regressor count of each width (None: no count fills the width).  Chow has 2 k regressors: only k = 8 fills one.
OLS_FULL = {R: R for R in OLS_WIDTHS}
ALS_FULL = {R: R for R in ALS_WIDTHS}
BOOT_FULL = {R: R for R in BOOT_WIDTHS}
CHOW_FULL = {2: 1, 4: 2, 8: 4, 16: 8}          # as k; K2 = 2 k = R


def groups(R):
    return THREADS // R


def three_workgroups(R):
    """Problems for three workgroups with a partial last one."""
    return 2 * groups(R) + 3


def boot_lds_bytes(ns, p, T):
    """launch_boot_r: NG groups x (T ns series + K ns exchange + 2 R Gauss-Jordan exchange) doubles."""
    R = boot_width(ns, p)
    return groups(R) * (T * ns + (1 + ns * p) * ns + 2 * R) * 8


def als_lds_bytes(r, T, N):
    """AlsLds<R>::doubles: factors, loadings, the good flags, NG exchange slots, 16 reduction slots."""
    R = als_width(r)
    return (T * R + N * R + N + groups(R) * 3 * R + 16) * 8


def quantile_lds_bytes(B):
    return pow2_ge(B) * 8


QUANTILE_MAX_B = 16384               # dfm_quantile_bands_dev


@contextlib.contextmanager
def _ols_by_normal_equations():
    """Inside the block als_oracle._ols solves X'X b = X'y instead of calling LAPACK least squares."""
    def normal(y, X):
        b = np.linalg.solve(X.T @ X, X.T @ y)
        return b, y - X @ b
    keep = ao._ols
    ao._ols = normal
    try:
        yield
    finally:
        ao._ols = keep


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


# ------------------------------------------------------------------------------------------------ OLS
# (K, T, note).  T stays in the tens of periods; the largest launch is the 259 problems of R = 2.
OLS_CASES = [
    (1, 40, ""),
    (2, 41, "K = R"),
    (3, 40, ""),
    (4, 43, "K = R"),
    (8, 45, "K = R"),
    (9, 50, ""),
    (16, 50, "K = R"),
    (32, 70, "K = R"),
    (33, 40, "T < R"),
    (64, 90, "K = R"),
]
OLS_NT_MIN_CASE = (3, 40)            # run once more with nt_min between the complete-row counts below
OLS_NT_MIN = 25                      # problem 5 has 20 complete rows (>= K: dropped by nt_min alone), problem 6 has 26
OLS_SHORT = 3                        # the problem with K - 1 complete rows: fewer than regressors


@functools.lru_cache(maxsize=None)
def ols_data(K, T, shared):
    """X [T, K] (shared, a constant last) or [P, T, K]; Y [T, P], one problem per column.  Missing cells are sparse enough
    that every regression keeps at least about 1.1 K rows: the point is the lane geometry, not the conditioning."""
    R = ols_width(K)
    P = three_workgroups(R)
    g = np.random.default_rng(1000 * K + 2 * T + int(shared))
    X = g.standard_normal((T, K)) if shared else g.standard_normal((P, T, K))
    if shared:
        X[:, -1] = 1.0
    Y = g.standard_normal((T, P)) + (X if shared else X[0]) @ g.standard_normal((K, P))
    Y[g.random((T, P)) < min(0.1, 0.15 * (T - K) / T)] = np.nan
    Y[:, OLS_SHORT] = np.nan
    Y[:K - 1, OLS_SHORT] = 1.0
    if (K, T) == OLS_NT_MIN_CASE:
        Y[:, 5] = g.standard_normal(T); Y[20:, 5] = np.nan
        Y[:, 6] = g.standard_normal(T); Y[26:, 6] = np.nan
    if not shared:
        X[2, :4, :] = np.nan                                       # missing regressor rows drop out too
        X[P - 1, T - 1, K - 1] = np.nan                            # ... in the partial workgroup, one cell only
    _frozen(X, Y)
    return X, Y


def _ols_reference(K, T, shared, nt_min, solve):
    X, Y = ols_data(K, T, shared)
    P = Y.shape[1]
    beta = np.full((P, K), np.nan); resid = np.full((T, P), np.nan)
    ssr = np.full(P, np.nan); tss = np.full(P, np.nan); nobs = np.zeros(P, dtype=np.int64)
    for p in range(P):
        Xp = X if shared else X[p]
        ok = ~np.isnan(Y[:, p]) & ~np.isnan(Xp).any(axis=1)
        nobs[p] = ok.sum()
        if nobs[p] < max(K, nt_min):
            continue
        b, e = solve(Y[ok, p], Xp[ok])
        beta[p], resid[ok, p], ssr[p] = b, e, e @ e
        d = Y[ok, p] - Y[ok, p].mean()
        tss[p] = d @ d
    out = dict(beta=beta, resid=resid, ssr=ssr, tss=tss, nobs=nobs)
    _frozen(*out.values())
    return out


@functools.lru_cache(maxsize=None)
def ols_reference(K, T, shared, nt_min=0):
    """`ols_skipmissing` per problem with als_oracle._ols on the complete rows; NaN where there are fewer than K or nt_min."""
    return _ols_reference(K, T, shared, nt_min, ao._ols)


@functools.lru_cache(maxsize=None)
def ols_reference_other(K, T, shared, nt_min=0):
    with _ols_by_normal_equations():
        return _ols_reference(K, T, shared, nt_min, ao._ols)


# ------------------------------------------------------------------------------------------------ bootstrap
# (ns, p, T, H, note); K = 1 + ns p regressors.
BOOT_CASES = [
    (1, 1, 60, 4, ""),
    (7, 1, 80, 5, "K = R"),
    (4, 2, 80, 6, ""),
    (5, 3, 100, 6, "K = R"),
    (3, 5, 100, 4, ""),
    (2, 8, 120, 4, ""),
    (1, 31, 200, 3, "K = R"),
    (8, 7, 160, 3, ""),
    (7, 9, 160, 3, "K = R"),
]
BOOT_FIRST_DRAWS = (0, 2 ** 32 - 5, 2 ** 40)       # the draws of a call cross 2^32 at the second; the third needs the high word
BOOT_SIGN_CASES = [(1, 1, 60, 4), (4, 2, 80, 6), (2, 8, 120, 4), (8, 7, 160, 3)]      # one per width
BOOT_SEED = 20160415
# the LDS refusal (launch_boot_r): at R = 8 the 32 groups share 160 KB, 640 doubles each.  The shape the notebook's VAR(1) of
# 4 factors would have, T = 222, is refused; the limit itself lies between T = 151 and T = 152 for ns = 4, p = 1.
BOOT_REFUSED = (4, 1, 222)
BOOT_LAST_FIT, BOOT_FIRST_REFUSED = (4, 1, 151), (4, 1, 152)


@functools.lru_cache(maxsize=None)
def var_data(ns, p, T):
    """A stationary VAR(p): lag l has weight 0.4 * 0.5^l on the identity (the weights sum below 0.8 for every p) plus a
    perturbation a tenth of that size, so the companion matrix stays inside the unit circle at p = 31 too."""
    g = np.random.default_rng(100000 + 1000 * ns + 10 * p + T)
    w = 0.4 * 0.5 ** np.arange(p)
    A = [w[l] * (np.eye(ns) + 0.1 * g.standard_normal((ns, ns)) / np.sqrt(ns)) for l in range(p)]
    chol = np.linalg.cholesky(np.eye(ns) + 0.3)
    y = np.zeros((T + 50, ns))
    for t in range(p, T + 50):
        y[t] = 0.2 + sum(A[l] @ y[t - 1 - l] for l in range(p)) + chol @ g.standard_normal(ns)
    y = np.ascontiguousarray(y[50:])                               # past the start-up
    _frozen(y)
    return y


@functools.lru_cache(maxsize=None)
def boot_signs(ns, p, T):
    B = three_workgroups(boot_width(ns, p))
    g = np.random.default_rng(5 + ns + 10 * p)
    signs = np.where(g.random((B, T)) < 0.5, -1.0, 1.0)
    signs[0] = 1.0                                                 # the identity draw
    _frozen(signs)
    return signs


def _boot_reference(ns, p, T, H):
    irf, beta, v = bo.var_bootstrap_irf(var_data(ns, p, T), p, H, boot_signs(ns, p, T))
    resid = np.zeros((T, ns)); resid[p:] = v["resid"][p:]
    point = ao.impulse_response(v["M"], v["Q"], v["G"], range(ns), H)
    out = dict(irf=irf, beta=beta, betahat=v["betahat"], resid=resid, point=point)
    _frozen(*out.values())
    return out


@functools.lru_cache(maxsize=None)
def boot_reference(ns, p, T, H):
    return _boot_reference(ns, p, T, H)


@functools.lru_cache(maxsize=None)
def boot_reference_other(ns, p, T, H):
    with _ols_by_normal_equations():
        return _boot_reference(ns, p, T, H)


# ------------------------------------------------------------------------------------------------ quantiles
QUANTILE_B = (1, 2, 255, 256, 257, 4096, 16384)
QUANTILE_S = (1, 7, 700)
QUANTILE_Q = (0.0, 1e-9, 0.05, 0.5, 0.84, 1.0)
# every B with the 7 column kinds below; one workgroup (S = 1) and 700 workgroups at the small B and around a power of two
QUANTILE_CASES = [(B, 7) for B in QUANTILE_B] + [(1, 1), (257, 1), (16384, 1), (1, 700), (256, 700), (257, 700)]
QUANTILE_KINDS = ("plain", "ties", "inf", "nan", "all_nan", "ties", "plain")   # column s is of kind s % 7
QUANTILE_FINITE = ("plain", "ties")


@functools.lru_cache(maxsize=None)
def quantile_data(B, S):
    g = np.random.default_rng(7 * B + S)
    x = g.standard_normal((B, S))
    for s in range(S):
        kind = QUANTILE_KINDS[s % 7]
        if kind == "ties":
            x[:, s] = np.round(2.0 * x[:, s]) / 2.0                # a handful of distinct values
        elif kind == "inf":
            x[0, s] = np.inf
            x[B - 1, s] = -np.inf                                  # (B = 1: the only draw is -inf)
            x[B // 2, s] = -np.inf if B > 2 else x[B // 2, s]
        elif kind == "nan":
            x[B // 3, s] = np.nan
        elif kind == "all_nan":
            x[:, s] = np.nan
    _frozen(x)
    return x


def quantile_reference(B, S):
    """The definition of tests/test_gpu_boot.py: the ceil(q B)-th smallest draw, NaN counted as +inf."""
    xs = np.sort(np.where(np.isnan(quantile_data(B, S)), np.inf, quantile_data(B, S)), axis=0)
    return np.stack([xs[min(max(int(np.ceil(q * B)) - 1, 0), B - 1)] for q in QUANTILE_Q])


def quantile_finite_columns(S):
    return [s for s in range(S) if QUANTILE_KINDS[s % 7] in QUANTILE_FINITE]


# ------------------------------------------------------------------------------------------------ Chow
CHOW_K = tuple(range(1, 9))
CHOW_QS = (0, 1, 6, 15)
CHOW_LENGTHS = (40, 63, 85, 108, 130)
CHOW_TRIM = 0.15                      # compute_qlr's ccut


def chow_break_range(T, k):
    """Break dates inside compute_qlr's trimming and at least 2 k + 2 rows from either end."""
    lo = max(int(np.floor(CHOW_TRIM * T)), 2 * k + 2)
    return lo, T - lo


@functools.lru_cache(maxsize=None)
def chow_data(k):
    """Five series of unequal length, each with a break and serially correlated errors; problems in shuffled series order,
    neighbouring problems walking through all four bandwidths."""
    g = np.random.default_rng(40 + k)
    ys, Xs = [], []
    for T in CHOW_LENGTHS:
        X = g.standard_normal((T, k)) + 0.3
        u = g.standard_normal(T)
        for t in range(1, T):
            u[t] += 0.5 * u[t - 1]
        y = X @ g.standard_normal(k) + u
        y[T // 2:] += X[T // 2:, 0]
        _frozen(X, y)
        ys.append(y); Xs.append(X)
    P = three_workgroups(chow_width(k))
    series = g.permutation(np.arange(P) % len(CHOW_LENGTHS))
    qs = np.array([CHOW_QS[(p + p // 4) % 4] for p in range(P)])    # rotates: no series keeps one bandwidth
    breaks = np.empty(P, dtype=np.int64)
    for p in range(P):
        lo, hi = chow_break_range(CHOW_LENGTHS[series[p]], k)
        breaks[p] = lo if p % 7 == 0 else hi if p % 7 == 1 else g.integers(lo, hi + 1)
    _frozen(series, breaks, qs)
    return tuple(ys), tuple(Xs), series, breaks, qs


def chow_other(y, X, q, T_break):
    """compute_chow with every normal-equations solve replaced by least squares: (W'W)^-1 = W^+ W^+' with the
    pseudo-inverse W^+ from numpy.linalg.lstsq, and the Wald form solved by lstsq too."""
    T, k = X.shape
    D = np.concatenate([np.zeros(T_break), np.ones(T - T_break)])
    W = np.column_stack([X, X * D[:, None]])
    Wp = np.linalg.lstsq(W, np.eye(T), rcond=None)[0]              # [2k, T]
    b = Wp @ y
    z = W * (y - W @ b)[:, None]
    kern = bk.form_kernel(q)
    v = kern[0] * z.T @ z
    for i in range(1, q + 1):
        c = z[i:].T @ z[:T - i]
        v += kern[i] * (c + c.T)
    WWi = Wp @ Wp.T
    V = WWi @ v @ WWi
    gm = b[k:]
    return float(gm @ np.linalg.lstsq(V[k:, k:], gm, rcond=None)[0])


def _chow_reference(k, stat):
    ys, Xs, series, breaks, qs = chow_data(k)
    out = np.array([stat(ys[s], Xs[s], int(q), int(tb)) for s, tb, q in zip(series, breaks, qs)])
    _frozen(out)
    return out


@functools.lru_cache(maxsize=None)
def chow_reference(k):
    return _chow_reference(k, bk.compute_chow)


@functools.lru_cache(maxsize=None)
def chow_reference_other(k):
    return _chow_reference(k, chow_other)


# ------------------------------------------------------------------------------------------------ standardize
STD_N = (1, 255, 256, 257, 600)
STD_T, STD_B, STD_MISS = 30, 3, 0.1


@functools.lru_cache(maxsize=None)
def standardize_data(N):
    """B panels with 10 % missing cells; series N // 2 of panel 1 has no observation at all."""
    g = np.random.default_rng(300 + N)
    x = 3.0 + 2.0 * g.standard_normal((STD_B, STD_T, N))
    x[g.random(x.shape) < STD_MISS] = np.nan
    x[1, :, N // 2] = np.nan
    _frozen(x)
    return x


# ------------------------------------------------------------------------------------------------ ALS
# (r, T, N, missing share, nt_min, note).  als_fits (als.hip) accepts every shape of the issue's list (T ~ 60, N ~ 64 is
# 40 KB of LDS at r = 32), so no shape had to be replaced: "asked" and "run" coincide and the table holds one of them.
# nt_min grows with r so that a series regression never has fewer rows than factors.
ALS_CASES = [
    (2, 60, 64, 0.10, 10, "r = R"),
    (4, 61, 63, 0.10, 10, "r = R"),
    (8, 60, 65, 0.10, 12, "r = R"),
    (16, 62, 67, 0.05, 24, "r = R"),
    (17, 60, 66, 0.05, 24, "first r of als_kernel<32>"),
    (32, 64, 67, 0.03, 40, "r = R = DFM_MAX_R"),
    (2, 60, 259, 0.10, 10, "r = R, three series chunks of NG = 128"),
    (4, 61, 131, 0.10, 10, "r = R, three series chunks of NG = 64"),
]
ALS_B = 3
ALS_MAX_ITER = 25
ALS_MIXED = dict(rmax=16, T=62, N=66, miss=0.05, nt_min=24, r_each=(16, 9, 1, 12), max_iter=25)   # r_each differs per run


def als_panel(seed, T, N, r, miss):
    """An unbalanced panel with r factors: sparse missing cells, three series that start T // 6 periods late, one series with
    five observations only (fewer than any nt_min: no loadings), and enough fully observed series for the PCA start."""
    g = np.random.default_rng(seed)
    f = g.standard_normal((T, r))
    x = f @ g.standard_normal((r, N)) + 0.7 * g.standard_normal((T, N))
    x[g.random((T, N)) < miss] = np.nan
    x[: T // 6, N - 3:] = np.nan
    x[:, N - 1] = np.nan
    x[:5, N - 1] = 1.0 + np.arange(5)
    nb = max(r + 2, N // 3)
    x[:, :nb] = np.where(np.isnan(x[:, :nb]), 0.3, x[:, :nb])
    return x


@functools.lru_cache(maxsize=None)
def als_reference(r, T, N, miss, nt_min, solver="normal"):
    """Per run of the batch: als_oracle.estimate_factor and the PCA start handed to the kernel."""
    out = []
    for b in range(ALS_B):
        x = als_panel(200 + 10 * r + b, T, N, r, miss)
        o = ao.estimate_factor(x, np.ones(N, int), 1, T, r, nt_min=nt_min, max_iter=ALS_MAX_ITER, solver=solver)
        o["F0"] = ao.pca_score(o["z"][:, ~np.isnan(o["z"]).any(axis=0)], r)
        _frozen(*o.values())
        out.append(o)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def als_mixed_reference(solver="normal"):
    c = ALS_MIXED
    x = als_panel(77, c["T"], c["N"], 6, c["miss"])
    z, _ = ao.standardize_data(x)
    F0 = ao.pca_score(z[:, ~np.isnan(z).any(axis=0)], c["rmax"])
    runs = tuple(ao.estimate_factor(x, np.ones(c["N"], int), 1, c["T"], r, nt_min=c["nt_min"], max_iter=c["max_iter"],
                                    solver=solver, compute_r2_flag=False) for r in c["r_each"])
    _frozen(z, F0)
    return z, F0, runs
