"""Expectation model of dfm_news_batch (include/dfm_hip.h) on the CPU: the three conditional means through the forecast's
expectation model (tests/forecast_expect.py), the news, and the weights by the header's construction -- the covariance panel on
the new vintage's mask, the oracle's smoother pass over it with mu0 = 0, w = (sd_i* / sd_i) (c - Lam g) / R.  Shared by
tests/test_news_cpu.py (checked against brute-force Gaussian conditioning) and tests/test_gpu_news.py."""
import numpy as np

from oracle import varp_oracle as vo
from tests.forecast_expect import expect as forecast_expect
from tests.simsmooth_expect import smoothed_mean


def horizon(targets, T):
    return max(0, max(int(t) for t, _ in targets) + 1 - T)


def state_covariances(A, Q, P0, p, rows):
    """Gamma_t = Var(z_t), t = 0 .. rows, of the companion state: Gamma_0 = P0, Gamma_t = M Gamma_{t-1} M' + Qk."""
    M, Qk = vo.companion(A, Q, p)
    G = [np.asarray(P0, float)]
    for _ in range(rows):
        G.append(M @ G[-1] @ M.T + Qk)
    return M, G


def cross_cov(M, Gam, u, v):
    """Cov(z_u, z_v) = M^(u-v) Gamma_v for u >= v, its transpose otherwise."""
    if u >= v:
        return np.linalg.matrix_power(M, u - v) @ Gam[v]
    return Gam[u] @ np.linalg.matrix_power(M, v - u).T


def covariance_panel(new, Lam, R, M, Gam, ts, i_s):
    """c_ti = lam_i' Cov(f_t+1, f_t*+1) lam_i* (+ R_i* on the target cell when observed) on the observed cells of new, NaN
    elsewhere."""
    T, N = new.shape
    r = Lam.shape[1]
    a = np.stack([cross_cov(M, Gam, t + 1, ts + 1)[:r, :r] @ Lam[i_s] for t in range(T)])
    c = a @ Lam.T
    if ts < T:
        c[ts, i_s] += R[i_s]
    return np.where(np.isnan(new), np.nan, c)


def expect(old, new, Lam, R, A, Q, mu0, P0, targets, p=1, mean=None, sd=None):
    """One replicate: old / new [T, N] (NaN = missing), A = [A_1 .. A_p] (r, r p), targets = G (t*, i*) pairs (0-based).
    Returns dict(yhat [3, G], impact [G, N], news [T, N], weight [G, T, N]) -- the outputs of dfm_news_batch."""
    old, new = np.asarray(old, float), np.asarray(new, float)
    T, N = new.shape
    r = Lam.shape[1]
    k = r * p
    H = horizon(targets, T)
    mu = np.zeros(N) if mean is None else np.asarray(mean, float)
    s = np.ones(N) if sd is None else np.asarray(sd, float)
    rev = np.where(np.isnan(old), np.nan, new)
    xh = [forecast_expect(x, Lam, R, A, Q, mu0, P0, H, p, mean=mean, sd=sd)["xhat"] for x in (old, rev, new)]
    yhat = np.array([[x[t, i] for t, i in targets] for x in xh])
    on = ~np.isnan(new)
    is_news = on & np.isnan(old)
    xnew = new if mean is None else mu + s * new
    news = np.where(is_news, xnew - xh[1][:T], 0.0)
    M, Gam = state_covariances(A, Q, P0, p, max(T, T + H))
    G = len(targets)
    weight = np.zeros((G, T, N))
    impact = np.zeros((G, N))
    for g, (ts, i_s) in enumerate(targets):
        c = covariance_panel(new, Lam, R, M, Gam, int(ts), int(i_s))
        gh = smoothed_mean(c, Lam, R, A, Q, np.zeros(k), P0, p)
        w = np.where(on, (s[i_s] / s) * (c - gh @ Lam.T) / R, 0.0)
        weight[g] = w
        impact[g] = (w * news).sum(axis=0)
    return dict(yhat=yhat, impact=impact, news=news, weight=weight)
