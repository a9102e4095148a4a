"""Expectation model of dfm_diffusion_eval_batch (include/dfm_hip.h) on the CPU: the windows, masks and standardisation of
tests/rolling_expect.py, the ALS sweeps of oracle/als_oracle.py (solver "normal") from the given start with the threshold tol W N,
every direct regression by np.linalg.lstsq on its complete cases, and the scoring rules as a plain loop.  Shared by
tests/test_diffusion_cpu.py (checked there against a second formulation) and tests/test_gpu_diffusion.py, which also take their cases
from here.

SENSITIVITY is the figure tests/test_diffusion_cpu.py::test_sensitivity_of_the_forecasts_to_the_factor_parity measures and holds
this constant against: the largest change of fc / win_sd when the oracle's converged factors of als_case() move by 1e-8 max|F|, the
parity tests/test_gpu_als.py grants the ALS."""
import numpy as np

from oracle import als_oracle as ao
from oracle import kalman_oracle as ko
from tests import rolling_expect as rx

ALS_PARITY = 1e-8                   # tests/test_gpu_als.py: factors and loadings of the ALS against the oracle
SENSITIVITY = 2e-7                  # measured 1.5e-7 (see above); the GPU suite's end-to-end bar is 10 x this


def als(z, F0, nt_min, max_iter, tol):
    """The oracle's sweeps on one standardised window from F0: (F, Lam, iters, ssr, ssr path).  max_iter = 0: the start itself."""
    W, N = z.shape
    F = np.array(F0, float)
    if max_iter == 0:
        return F, np.full((N, F.shape[1]), np.nan), 0, np.nan, np.zeros(0)
    obs = ~np.isnan(z)
    ssr, path, lam = 0.0, [], None
    for _ in range(max_iter):
        ssr_old = ssr
        lam = ao._lambda_step(z, obs, F, nt_min, "normal")
        F, ssr = ao._factor_step(z, obs, lam, "normal")
        path.append(ssr)
        if not abs(ssr_old - ssr) >= tol * W * N:
            break
    return F, lam, len(path), ssr, np.array(path)


def design(z, F, i, l, h, q):
    """Rows s = max(0, l + q - 1) .. W - 1 - l - h of regression (i, h): (U [rows, K], y [rows], complete [rows])."""
    W = z.shape[0]
    s = np.arange(max(0, l + q - 1), W - l - h)
    if s.size == 0:
        return np.zeros((0, 1 + F.shape[1] + q)), np.zeros(0), np.zeros(0, bool)
    U = np.column_stack([np.ones(s.size), F[s]] + [z[s - l - m, i] for m in range(q)])
    y = z[s + h, i]
    return U, y, ~np.isnan(y) & ~np.isnan(U).any(axis=1)


def origin_row(z, F, i, l, q):
    """u_{W-1} of series i: NaN where an own lag is missing or lies in front of the window."""
    W = z.shape[0]
    lagv = [z[W - 1 - l - m, i] if W - 1 - l - m >= 0 else np.nan for m in range(q)]
    return np.concatenate([[1.0], F[W - 1], lagv])


def regress_window(z, F, mu, sd, H, q, lags, nt_min):
    """Every regression of one window: fc, fc_ar, fvar [H+1, N] (data units), beta [H+1, N, K], nobs_reg [H+1, N]."""
    W, N = z.shape
    r = F.shape[1]
    K = 1 + r + q
    fc = np.full((H + 1, N), np.nan); fa = np.full((H + 1, N), np.nan); fv = np.full((H + 1, N), np.nan)
    beta = np.full((H + 1, N, K), np.nan); nobs = np.zeros((H + 1, N), dtype=np.int32)
    if not np.all(np.isfinite(F)):
        return fc, fa, fv, beta, nobs
    ar = np.r_[0, 1 + r:K]
    for i in range(N):
        l = int(lags[i])
        u0 = origin_row(z, F, i, l, q)
        for h in range(H + 1):
            if h + l < 1:
                continue
            U, y, ok = design(z, F, i, l, h, q)
            n = int(ok.sum())
            nobs[h, i] = n
            if n < max(nt_min, K):
                continue
            U, y = U[ok], y[ok]
            b = np.linalg.lstsq(U, y, rcond=None)[0]
            e = y - U @ b
            ba = np.linalg.lstsq(U[:, ar], y, rcond=None)[0]
            beta[h, i] = b
            fc[h, i] = mu[i] + sd[i] * (b @ u0)
            fa[h, i] = mu[i] + sd[i] * (ba @ u0[ar])
            if n > K:
                fv[h, i] = sd[i] ** 2 * float(e @ e) / (n - K)
    return fc, fa, fv, beta, nobs


def score(x, origins, fc, fc_ar, fvar, mean):
    """err, err_ar, err_std [O, H+1, N] (NaN where not scored) and msfe, msfe_ar, msfe0, cnt [H+1, N], the sums in origin order."""
    x = np.asarray(x, float)
    T, N = x.shape
    O, H1, _ = fc.shape
    err = np.full((O, H1, N), np.nan); ea = np.full((O, H1, N), np.nan); es = np.full((O, H1, N), np.nan)
    sse = np.zeros((H1, N)); ssa = np.zeros((H1, N)); sse0 = np.zeros((H1, N)); cnt = np.zeros((H1, N), dtype=np.int32)
    for b, o in enumerate(origins):
        for h in range(H1):
            if o + h >= T:
                continue
            for i in range(N):
                if np.isnan(x[o + h, i]) or not np.isfinite(fc[b, h, i]):
                    continue
                e, a, e0 = x[o + h, i] - fc[b, h, i], x[o + h, i] - fc_ar[b, h, i], x[o + h, i] - mean[b, i]
                err[b, h, i], ea[b, h, i] = e, a
                with np.errstate(invalid="ignore", divide="ignore"):
                    es[b, h, i] = e / np.sqrt(fvar[b, h, i])
                sse[h, i] += e * e; ssa[h, i] += a * a; sse0[h, i] += e0 * e0; cnt[h, i] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        ms = lambda s: np.where(cnt > 0, s / cnt, np.nan)
        return dict(err=err, err_ar=ea, err_std=es, msfe=ms(sse), msfe_ar=ms(ssa), msfe0=ms(sse0), cnt=cnt)


def start_windows(F_start, origins, W):
    """The start of every window [O, W, r]: cut from one [T, r] path, or the [O, W, r] given."""
    F_start = np.asarray(F_start, float)
    if F_start.ndim == 3:
        return F_start.copy()
    return np.stack([F_start[o - W + 1:o + 1] for o in origins])


def expect(x, origins, W, H, F_start, q, lags=None, nt_min=0, max_iter=0, tol=0.0, F=None, only=None):
    """The whole record.  F: factors [O, W, r] to use in place of the ALS's (the regressions at the factors a call returned).  only:
    the windows (indices) that are computed -- the others keep NaN / 0; the scores only when `only` is None.  Returns dict(win, mean,
    sd, nobs, F, Lam, iters, ssr, paths, fc, fc_ar, fvar, beta, nobs_reg, err, err_ar, err_std, msfe, msfe_ar, msfe0, cnt)."""
    origins = np.asarray(origins, dtype=int)
    x = np.asarray(x, float)
    N = x.shape[1]
    lg = np.zeros(N, dtype=int) if lags is None else np.asarray(lags, dtype=int)
    mu, sd, n, z = rx.standardise(rx.windows(x, origins, W, lags))
    F0 = start_windows(F_start, origins, W)
    O, r = origins.size, F0.shape[2]
    K = 1 + r + q
    out = dict(win=z, mean=mu, sd=sd, nobs=n, F=np.full((O, W, r), np.nan), Lam=np.full((O, N, r), np.nan),
               iters=np.zeros(O, dtype=np.int32), ssr=np.full(O, np.nan), paths=[None] * O, fc=np.full((O, H + 1, N), np.nan),
               fc_ar=np.full((O, H + 1, N), np.nan), fvar=np.full((O, H + 1, N), np.nan), beta=np.full((O, H + 1, N, K), np.nan),
               nobs_reg=np.zeros((O, H + 1, N), dtype=np.int32))
    for b in (range(O) if only is None else only):
        if F is None:
            out["F"][b], out["Lam"][b], out["iters"][b], out["ssr"][b], out["paths"][b] = als(z[b], F0[b], nt_min, max_iter, tol)
        else:
            out["F"][b] = F[b]
        out["fc"][b], out["fc_ar"][b], out["fvar"][b], out["beta"][b], out["nobs_reg"][b] = \
            regress_window(z[b], out["F"][b], mu[b], sd[b], H, q, lg, nt_min)
    if only is None:
        out.update(score(x, origins, out["fc"], out["fc_ar"], out["fvar"], mu))
    return out


# ---- the cases of tests/test_gpu_diffusion.py (the CPU suite checks their conditioning and coverage) ----------------------------
RQ = [(1, 0), (2, 1), (4, 4), (8, 4), (8, 7), (8, 23)]        # K = 2, 4, 9, 13, 16, 32: every R, both sides of the 4 / 8 and 8 / 16 pads
NS = [1, 7, 16, 17, 65]                                       # the series block is 16
HS = [0, 1, 4]
VARIANTS = ("none", "mod4", "max")


def windows_of(r, q):
    """W = 24 and 33; K = 32 must keep complete rows, so (8, 23) runs at W = 80 only."""
    return [80] if (r, q) == (8, 23) else [24, 33]


def refused(r, q, W, H):
    """What DFM_E_DIMS refuses of the grid: W < K + q + H + 2."""
    return W < 1 + r + q + q + H + 2


def kernel_nt_min(r, q):
    return 1 + r + q + 4                                      # a few rows more than regressors: the Gram matrices stay conditioned


def kernel_case(N, W, r, q, variant):
    """A raw panel of T = W + 12 rows, origins at the first full window, an uneven step and T - 1, random finite start factors (one
    path, and the same cut per window); 10 % missing cells (series 0 keeps all its cells where q > 4: with that many own lags
    hardly a row is complete otherwise), one series at the largest lag (N >= 3: series 1) and one unobserved on every target row
    (N >= 3: the last).  Returns (x, origins, lags, F_path [T, r], min_obs)."""
    T = W + 12
    min_obs = r + 1
    rs = min(2, N)
    z, _ = ko.synth_replicate(11, N, T, rs)
    rng = np.random.default_rng([N, W, r, q])
    x = z * rng.uniform(0.5, 3.0, N) + rng.uniform(-2.0, 2.0, N)
    origins = np.array([W - 1, W + 1, W + 4, T - 1])
    j_lag, j_dead = (1, N - 1) if N >= 3 else (None, None)
    lags = {"none": None, "mod4": np.arange(N) % 4, "max": np.zeros(N, dtype=int)}[variant]
    if variant == "max" and j_lag is not None:
        lags[j_lag] = W - min_obs
    if lags is not None and j_dead is not None:
        lags[j_dead] = 0
    miss = rng.random((T, N)) < 0.1
    if q > 4:
        miss[:, 0] = False
    if j_lag is not None:
        miss[:, j_lag] = False
    if j_dead is not None:
        miss[:, j_dead] = False
        miss[W:W + 9, j_dead] = True                          # every target row o + h, h = 1 .. 4, of the origins before T - 1
    xm = np.where(miss, np.nan, x)
    thin = ((~np.isnan(rx.windows(xm, origins, W, lags))).sum(axis=1) < min_obs).any(axis=0)
    xm[:, thin] = x[:, thin]                                  # (a series the draw left too thin for a window keeps all its cells)
    assert not rx.window_fails(rx.windows(xm, origins, W, lags), min_obs)
    F = np.random.default_rng([7, N, W, r]).standard_normal((T, r))
    return xm, origins, lags, F, min_obs


def als_case():
    """The inputs of the ALS cases: (x, origins, W, H, q, lags, nt_min, F_path [T, r])."""
    N, T, r = 12, 70, 2
    z, _ = ko.synth_replicate(0, N, T, r, missing=0.05)
    rng = np.random.default_rng(7)
    x = z * rng.uniform(0.5, 3.0, N) + rng.uniform(-2.0, 2.0, N)
    W, H, q = 40, 3, 2
    origins = np.arange(39, 67, 3)
    lags = np.arange(N) % 3
    zf, _ = ao.standardize_data(x)
    F = ao.pca_score(np.nan_to_num(zf), r)
    return x, origins, W, H, q, lags, 8, F


ALS_TOL = 1e-8                                                # the tol of the API's default model (m.tol of the notebook's DFMModel)
