"""Expectation model of dfm_rolling_eval_batch (include/dfm_hip.h) on the CPU: the windows, their vintage masks and standardisation,
the start rescale, the oracle's EM per window (oracle/kalman_oracle.py at p = 1, oracle/varp_oracle.py beyond), the forecasts of
tests/forecast_expect.expect on each window and the scoring rules.  Shared by tests/test_rolling_eval_cpu.py (checked there against
brute-force conditioning and a naive loop) and tests/test_gpu_rolling_eval.py."""
import numpy as np

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests.forecast_expect import expect as fc_expect

KEYS = ("Lam", "R", "Avar", "Q", "mu0", "P0")


def windows(x, origins, W, lags=None):
    """The raw vintages [O, W, N]: rows o - W + 1 .. o of x, NaN where t > o - lag_i (and where x is)."""
    x = np.asarray(x, float)
    N = x.shape[1]
    lg = np.zeros(N, dtype=int) if lags is None else np.asarray(lags, dtype=int)
    out = []
    for o in origins:
        w = x[o - W + 1:o + 1].copy()
        hidden = np.arange(W)[:, None] > (W - 1 - lg)[None, :]
        w[hidden] = np.nan
        out.append(w)
    return np.stack(out)


def standardise(win):
    """Mean, population s.d. and count of every window's visible cells ([O, N] each) and the standardised windows."""
    obs = ~np.isnan(win)
    n = obs.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.where(obs, win, 0.0).sum(axis=1) / n
        d = np.where(obs, win - mu[:, None, :], 0.0)
        sd = np.sqrt((d * d).sum(axis=1) / n)
        z = (win - mu[:, None, :]) / sd[:, None, :]
    return mu, sd, n.astype(np.int32), z


def window_fails(win, min_obs):
    """DFM_E_WINDOW: a series of a window with fewer than min_obs visible cells, or whose visible cells are all equal."""
    obs = ~np.isnan(win)
    const = np.where(obs, win, np.inf).min(axis=1) == np.where(obs, win, -np.inf).max(axis=1)
    return bool((obs.sum(axis=1) < min_obs).any() or const.any())


def rescale_start(start, sd, sd_start=None):
    """The start of every window: start [n_start, ..] by KEYS broadcast (n_start = 1) or copied, the loadings and variances
    rescaled by sc = sd_start / win_sd (None: 1)."""
    O, N = sd.shape
    out = {}
    for k in KEYS:
        a = np.asarray(start[k], float)
        out[k] = np.ascontiguousarray(np.broadcast_to(a, (O,) + a.shape[1:])).copy()
    if sd_start is not None:
        sc = np.asarray(sd_start, float)[None, :] / sd
        out["Lam"] = out["Lam"] * sc[:, :, None]
        out["R"] = out["R"] * (sc * sc)
    return out


def em_window(z, params, p, max_iter, tol):
    """The oracle's EM on one standardised window: (params by KEYS, loglik path)."""
    if max_iter == 0:
        return {k: np.array(params[k], float) for k in KEYS}, np.zeros(0)
    if p == 1:
        q, path, _ = ko.em(z, dict(Lam=params["Lam"], R=params["R"], A=params["Avar"], Q=params["Q"], mu0=params["mu0"],
                                   P0=params["P0"]), max_iter=max_iter, tol=tol)
        return dict(Lam=q["Lam"], R=q["R"], Avar=q["A"], Q=q["Q"], mu0=q["mu0"], P0=q["P0"]), path
    q, path, _ = vo.em_varp(z, {k: params[k] for k in KEYS}, p, max_iter, tol)
    return q, path


def forecasts(z, params, mu, sd, H, p):
    """fc, fvar [O, H+1, N] in data units at the given per-window parameters ([O, ..] by KEYS) and standardised windows."""
    O, W, N = z.shape
    fc, fv = np.empty((O, H + 1, N)), np.empty((O, H + 1, N))
    for b in range(O):
        e = fc_expect(z[b], *[params[k][b] for k in KEYS], H, p=p, mean=mu[b], sd=sd[b])
        fc[b], fv[b] = e["xhat"][W - 1:], e["xvar"][W - 1:]
    return fc, fv


def score(x, origins, lags, fc, fvar, mean):
    """err, err_std [O, H+1, N] (NaN where not scored) and msfe, msfe0, cnt [H+1, N], the sums in origin order."""
    x = np.asarray(x, float)
    T, N = x.shape
    O, H1, _ = fc.shape
    lg = np.zeros(N, dtype=int) if lags is None else np.asarray(lags, dtype=int)
    err = np.full((O, H1, N), np.nan); es = np.full((O, H1, N), np.nan)
    sse = np.zeros((H1, N)); sse0 = np.zeros((H1, N)); cnt = np.zeros((H1, N), dtype=np.int32)
    for b, o in enumerate(origins):
        for h in range(H1):
            if o + h >= T:
                continue
            hidden = np.ones(N, bool) if h > 0 else lg > 0
            ok = hidden & ~np.isnan(x[o + h])
            e = x[o + h] - fc[b, h]
            err[b, h, ok] = e[ok]
            es[b, h, ok] = e[ok] / np.sqrt(fvar[b, h, ok])
            e0 = x[o + h] - mean[b]
            sse[h, ok] += e[ok] * e[ok]; sse0[h, ok] += e0[ok] * e0[ok]; cnt[h, ok] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        msfe = np.where(cnt > 0, sse / cnt, np.nan); msfe0 = np.where(cnt > 0, sse0 / cnt, np.nan)
    return dict(err=err, err_std=es, msfe=msfe, msfe0=msfe0, cnt=cnt)


def expect(x, origins, W, H, start, lags=None, sd_start=None, p=1, max_iter=0, tol=0.0, only=None):
    """The whole record.  start: dict by KEYS with a leading axis of 1 or O.  only: the windows (indices) whose EM is run -- the
    others keep NaN parameters and forecasts (a test that compares a few windows need not pay for all).  Returns dict(win, mean,
    sd, nobs, start, params, paths, iters, fc, fvar, err, err_std, msfe, msfe0, cnt); the scores only when `only` is None."""
    origins = np.asarray(origins, dtype=int)
    raw = windows(x, origins, W, lags)
    mu, sd, n, z = standardise(raw)
    st = rescale_start(start, sd, sd_start)
    O = origins.size
    which = range(O) if only is None else only
    params = {k: np.full_like(st[k], np.nan) for k in KEYS}
    paths, iters = [None] * O, np.zeros(O, dtype=np.int32)
    for b in which:
        q, path = em_window(z[b], {k: st[k][b] for k in KEYS}, p, max_iter, tol)
        for k in KEYS:
            params[k][b] = q[k]
        paths[b], iters[b] = path, len(path)
    N = z.shape[2]
    fc, fv = np.full((O, H + 1, N), np.nan), np.full((O, H + 1, N), np.nan)
    idx = list(which)
    f1, v1 = forecasts(z[idx], {k: params[k][idx] for k in KEYS}, mu[idx], sd[idx], H, p)
    fc[idx], fv[idx] = f1, v1
    out = dict(win=z, mean=mu, sd=sd, nobs=n, start=st, params=params, paths=paths, iters=iters, fc=fc, fvar=fv)
    if only is None:
        out.update(score(x, origins, lags, fc, fv, mu))
    return out


def em_parity_case():
    """The inputs of the EM parity case of tests/test_gpu_rolling_eval.py, whose stop decisions tests/test_rolling_eval_cpu.py
    holds away from the tolerance: (x, origins, W, H, lags, start by KEYS with a leading axis of 1)."""
    z, _ = ko.synth_replicate(0, 12, 70, 2, missing=0.05)
    rng = np.random.default_rng(7)
    x = z * rng.uniform(0.5, 3.0, 12) + rng.uniform(-2.0, 2.0, 12)
    W, H = 40, 3
    origins = np.arange(39, 67, 3)
    lags = np.arange(12) % 3
    _, _, _, z0 = standardise(windows(x, origins[:1], W, lags))
    q, _ = ko.pca_init(np.nan_to_num(z0[0]), 2)
    start = dict(Lam=q["Lam"][None], R=q["R"][None], Avar=q["A"][None], Q=q["Q"][None], mu0=q["mu0"][None], P0=q["P0"][None])
    return x, origins, W, H, lags, start
