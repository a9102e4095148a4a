"""NumPy model of the mixed-frequency DFM (include/dfm_hip.h: dfm_ks_pass_mf_batch / dfm_em_mf_batch), test infrastructure only:

    x_it = lam_i' g_it + e_it,  g_it = sum_{l<L} w_il f_{t-l},  e_it ~ N(0, R_i);   f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t

on the companion state z_t = (f_t, .., f_{t-m+1}), m = max(p, L): loadings [w_i0 lam_i, .., w_i,L-1 lam_i, 0..], transition of
[A_1..A_p, 0], innovation covariance [Q 0; 0 0].  The generic pass and `companion` come from the oracles, as in news_expect.py.
"""
from __future__ import annotations

import numpy as np

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo

WEIGHTS = {"m": (1.0,), "q_flow": (1 / 3, 2 / 3, 1.0, 2 / 3, 1 / 3), "q_avg": (1 / 3, 1 / 3, 1 / 3)}


def weight_rows(kinds, L=None):
    """[N][L] weights from a list of "m" / "q_flow" / "q_avg" (L: at least the longest pattern)."""
    L = max(len(WEIGHTS[k]) for k in kinds) if L is None else L
    W = np.zeros((len(kinds), L))
    for i, k in enumerate(kinds):
        W[i, :len(WEIGHTS[k])] = WEIGHTS[k]
    return W


def mf_loadings(Lam, W, m):
    """Lam (N, r), W (N, L) -> (N, r m): [w_i0 lam_i, .., w_i,L-1 lam_i, 0..]."""
    N, r = Lam.shape
    L = W.shape[1]
    out = np.zeros((N, m, r))
    out[:, :L] = W[:, :, None] * Lam[:, None, :]
    return out.reshape(N, m * r)


def expanded(Lam, W, Avar, Q):
    """(LamK, M, Qk, m) of the expanded model."""
    r = Lam.shape[1]
    p = Avar.shape[1] // r
    m = max(p, W.shape[1])
    Ak = np.zeros((r, r * m)); Ak[:, :r * p] = Avar
    M, Qk = vo.companion(Ak, Q, m)
    return mf_loadings(Lam, W, m), M, Qk, m


def kfs_pass_mf(x, Lam, R, W, Avar, Q, mu0, P0):
    LamK, M, Qk, _ = expanded(Lam, W, Avar, Q)
    return ko.kfs_pass(np.asarray(x, float), LamK, R, M, Qk, mu0, P0, lag_one=True)


def em_step_mf(x, Lam, R, W, Avar, Q, mu0, P0):
    """One EM iteration; returns (new parameters, log-likelihood at the entering parameters, the pass's dict)."""
    x = np.asarray(x, float)
    T, N = x.shape
    r = Lam.shape[1]
    p = Avar.shape[1] // r
    L = W.shape[1]
    m = max(p, L)
    out = kfs_pass_mf(x, Lam, R, W, Avar, Q, mu0, P0)
    zs, Ps, Pl = out["f_smooth"], out["P_smooth"], out["P_lag"]
    z0, P0s = out["f0_smooth"], out["P0_smooth"]
    Ez = zs[:, :, None] * zs[:, None, :] + Ps
    S11 = Ez.sum(0)
    S00 = S11 - Ez[-1] + (np.outer(z0, z0) + P0s)
    zprev = np.vstack([z0[None, :], zs[:-1]])
    S10 = (zs[:, :, None] * zprev[:, None, :] + Pl).sum(0)
    ka = r * p
    A_new = np.linalg.solve(S00[:ka, :ka].T, S10[:r, :ka].T).T
    Q_new = (S11[:r, :r] - A_new @ S10[:r, :ka].T) / T
    Q_new = 0.5 * (Q_new + Q_new.T)
    zb = zs.reshape(T, m, r)[:, :L]                                # E f_{t-l}
    Eb = Ez.reshape(T, m, r, m, r)[:, :L, :, :L, :]                # E[f_{t-l} f_{t-l'}']
    obs = ~np.isnan(x)
    Lam_new = Lam.copy(); R_new = R.copy()
    for i in range(N):
        o = obs[:, i]
        n = int(o.sum())
        if n < r + 1:
            continue
        w = W[i]
        G = np.einsum("l,tlcmd,m->cd", w, Eb[o], w)
        b = np.einsum("l,tlc->tc", w, zb[o]).T @ x[o, i]
        try:                                                       # a G_i that is not positive definite keeps lam_i and R_i
            np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            continue
        lam = np.linalg.solve(G, b)
        Lam_new[i] = lam
        R_new[i] = ((x[o, i] ** 2).sum() - 2.0 * lam @ b + lam @ G @ lam) / n
    new = dict(Lam=Lam_new, R=R_new, Avar=A_new, Q=Q_new, mu0=z0.copy(), P0=0.5 * (P0s + P0s.T))
    return new, out["loglik"], out


def em_mf(x, params, W, max_iter=10, tol=0.0):
    """EM loop with ko.em's bookkeeping (path[k] = log-likelihood at the parameters entering iteration k)."""
    cur = {k: np.array(v, float) for k, v in params.items()}
    path = []
    out = None
    for it in range(max_iter):
        new, ll, out = em_step_mf(x, W=W, **cur)
        path.append(ll)
        if it >= 1 and tol > 0.0:
            if (path[-1] - path[-2]) / (0.5 * (abs(path[-1]) + abs(path[-2]))) < tol:
                break
        cur = new
    return cur, np.array(path), out


def mf_start(x, W, r, p):
    """A rough start from the panel: PCA of the zero-filled monthly series, loadings of every series by a
    regression on the aggregated PCA factors over its observed cells, VAR(p) by OLS, a loose P0."""
    T, N = x.shape
    L = W.shape[1]
    m = max(p, L)
    first = (W[:, 0] == 1.0) & np.all(W[:, 1:] == 0.0, axis=1)    # the monthly series (all of them if none is)
    if not first.any():
        first[:] = True
    xm = np.where(np.isnan(x[:, first]), 0.0, x[:, first])
    _, F = ko.pca_init(xm, r)
    Lam = np.zeros((N, r)); R = np.ones(N)
    for i in range(N):
        g = sum(W[i, l] * np.vstack([np.zeros((l, r)), F[:T - l]]) for l in range(L))
        o = ~np.isnan(x[:, i]); o[:L - 1] = False
        if o.sum() < r + 1:
            continue
        lam = np.linalg.lstsq(g[o], x[o, i], rcond=None)[0]
        Lam[i] = lam
        R[i] = max(np.mean((x[o, i] - g[o] @ lam) ** 2), 0.05)
    Z = np.hstack([F[p - 1 - l:T - l] for l in range(p)])
    Y, Xl = F[p:], Z[:-1]
    Avar = np.linalg.solve(Xl.T @ Xl, Xl.T @ Y).T
    e = Y - Xl @ Avar.T
    Q = e.T @ e / (T - p); Q = 0.5 * (Q + Q.T)
    Zm = np.hstack([F[m - 1 - l:T - l] for l in range(m)])
    P0 = Zm.T @ Zm / Zm.shape[0] + 1e-3 * np.eye(r * m)
    return dict(Lam=Lam, R=R, Avar=Avar, Q=Q, mu0=np.zeros(r * m), P0=0.5 * (P0 + P0.T))


def synth_mf(b, Nm, Nq, T, r, p, kind="q_flow", missing=0.0, ragged=0, interleave=False, seed=ko.SEED0, L=None):
    """Seeded mixed-frequency panel: Nm monthly series, Nq quarterly ones of `kind` (NaN outside every third month), optional
    random missing cells in the MONTHLY series and a ragged edge of up to `ragged` trailing months.  `kind` may be a list
    (one entry per quarterly series).  Returns (x, W, start); interleave=True mixes the two groups in the series order."""
    rng = np.random.default_rng([seed, b, p, 11])
    kinds = [kind] * Nq if isinstance(kind, str) else list(kind)
    W = weight_rows(["m"] * Nm + kinds, L)
    L = W.shape[1]
    N = Nm + Nq
    wl = 0.5 ** np.arange(1, p + 1); wl = 0.8 * wl / wl.sum()
    Avar = np.hstack([np.diag(np.linspace(0.6, 1.0, r)) * wl[l] * (1.0 if l % 2 == 0 else -1.0) for l in range(p)])
    f = np.zeros((T + 60, r))
    for t in range(p, T + 60):
        f[t] = Avar @ np.concatenate([f[t - 1 - l] for l in range(p)]) + np.sqrt(np.linspace(0.5, 1.0, r)) * rng.standard_normal(r)
    Lam = rng.standard_normal((N, r))
    g = np.stack([sum(W[i, l] * f[60 - l:T + 60 - l] for l in range(L)) @ Lam[i] for i in range(N)], axis=1)
    x = g + np.sqrt(rng.uniform(0.3, 1.0, N)) * rng.standard_normal((T, N))
    x = (x - x.mean(0)) / x.std(0)
    if missing > 0.0:
        x[:, :Nm] = np.where(rng.random((T, Nm)) < missing, np.nan, x[:, :Nm])
    if ragged > 0:
        for i in range(Nm):
            k = int(rng.integers(0, ragged + 1))
            if k:
                x[T - k:, i] = np.nan
    x[np.arange(T) % 3 != 2, Nm:] = np.nan
    if interleave:
        perm = rng.permutation(N)
        x, W = x[:, perm], W[perm]
    start = mf_start(x, W, r, p)
    return x, np.ascontiguousarray(W), start
