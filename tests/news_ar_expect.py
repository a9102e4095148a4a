"""Expectation model of dfm_news_ar_batch (include/dfm_hip.h; csrc/news_ar.hip) on the CPU, two texts:

  expect        the three conditional means through forecast_ar_expect.expect, the news against the revised-old xhat, and the weights
                by the construction the library runs: the covariance of every quasi-differenced cell with the target from the
                structured recursion (qc_panel), the oracle's smoother pass (oracle.kalman_oracle.kfs_pass) over it with mu0 = 0,
                and the adjoint of the quasi-difference on its residuals;
  brute_force   the joint Gaussian of every output cell, horizon included, from the model's OWN recursion (no quasi-differencing, no
                smoother: forecast_ar_expect.brute_force extended to masked vintages), conditioned densely: the three means,
                Sigma^-1 c on the cells of new and Cov(y, I) Var(I)^-1 on the news cells.

Vintages are EDGE-SHAPED (vintages()): every series observed on panel rows 0 .. L_i, L_i >= 2q - 1.  Parameters come from
forecast_ar_expect.synth with the factor VAR rescaled to spectral radius <= 0.9 (stable()): the raw start can be explosive, and a
joint covariance with entries of 1e5 leaves brute-force conditioning its own error of 1e-10.
Shared by tests/test_news_ar_cpu.py and tests/test_gpu_news_ar.py."""
import numpy as np

from oracle import ar_oracle as ao
from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests import forecast_ar_expect as fe

KEYS = fe.KEYS


# ---------------------------------------------------------------------------------------------------- inputs
def stable(st, bound=0.9):
    """st with Avar rescaled (A_l -> c^l A_l scales every eigenvalue of the companion matrix by c) to spectral radius <= bound."""
    Avar, r = st["Avar"], st["Lam"].shape[1]
    p = Avar.shape[1] // r
    M, _ = vo.companion(Avar, st["Q"], p)
    rad = np.abs(np.linalg.eigvals(M)).max()
    if rad <= bound:
        return st
    c = bound / rad
    A = np.hstack([Avar[:, l * r:(l + 1) * r] * c ** (l + 1) for l in range(p)])
    return dict(st, Avar=A)


def synth(b, N, T, r, p, q, seed=ko.SEED0):
    """(x [T, N] balanced, st with a stable factor VAR, v0 [N])."""
    Ts = max(T, 3 * r + 12)                                          # the start's PCA wants a few rows; short panels are cut from it
    x, st, v0 = fe.synth(b, max(N, r + 2), Ts, r, p, q, seed=seed)
    st = dict(st, Lam=st["Lam"][:N], sig2=st["sig2"][:N], rho=st["rho"][:N])
    return np.ascontiguousarray(x[:T, :N]), stable(st), v0[:N]


def vintages(x, L_old, L_new, revised=()):
    """old / new [T, N] from the balanced x: series i is observed on rows 0 .. L_old[i] / 0 .. L_new[i] (-1: never);
    revised: (t, i, delta) cells whose value in old is x - delta."""
    T, N = x.shape
    rows = np.arange(T)[:, None]
    old = np.where(rows <= np.asarray(L_old)[None, :], x, np.nan)
    new = np.where(rows <= np.asarray(L_new)[None, :], x, np.nan)
    for t, i, delta in revised:
        old[t, i] -= delta
    return old, new


def horizon(T, targets):
    return max(0, max(int(t) for t, _ in targets) + 1 - T)


# ---------------------------------------------------------------------------------------------------- the covariance panel
def model_matrices(st):
    Lam, rho, Avar, Q = st["Lam"], st["rho"], st["Avar"], st["Q"]
    r, q = Lam.shape[1], rho.shape[1]
    m = ao.state_lags(Avar.shape[1] // r, q)
    Ak = np.zeros((r, r * m))
    Ak[:, :Avar.shape[1]] = Avar
    M, Qk = vo.companion(Ak, Q, m)
    return M, Qk, ao.ar_loadings(Lam, rho, m)


def impulse(rho, n):
    """psi_0 .. psi_{n-1} of e_t = sum_l rho_l e_{t-l} + eps_t."""
    psi = np.zeros(n)
    for j in range(n):
        psi[j] = 1.0 if j == 0 else sum(rho[l] * psi[j - 1 - l] for l in range(len(rho)) if j - 1 - l >= 0)
    return psi


def qc_panel(st, ts, i_s, rows):
    """Cov(xq_ti, y) for t < rows and every series, y the target cell of OUTPUT row ts and series i_s, xq the quasi-differenced
    cells given the first q panel rows: [rows, N].  u backwards from the target, Gamma / v forwards."""
    M, Qk, Hl = model_matrices(st)
    k = M.shape[0]
    h = Hl[i_s]
    psi = impulse(st["rho"][i_s], ts + 1)
    u = np.zeros((max(ts, rows) + 2, k))
    for t in range(ts, -1, -1):
        u[t] = M.T @ u[t + 1] + psi[ts - t] * h
    G, v = st["P0"], np.zeros(k)
    out = np.empty((rows, Hl.shape[0]))
    for t in range(rows):
        G = M @ G @ M.T + Qk
        src = psi[ts - t] if t <= ts else 0.0
        d = M @ v + G @ u[t]
        v = M @ v + src * (G @ h)
        out[t] = Hl @ d
        out[t, i_s] += src * st["sig2"][i_s]
    return out


def weights(new, st, ts, i_s, sd=None):
    """w = d y_new / d x on the cells of new in the sample's output rows [T - q, N] (0 elsewhere), data units with sd."""
    T, N = new.shape
    q = st["rho"].shape[1]
    ns = T - q
    M, Qk, Hl = model_matrices(st)
    obs = ~np.isnan(ao.quasi_difference(new, st["rho"]))
    qc = np.where(obs, qc_panel(st, ts, i_s, ns), np.nan)
    g = ko.kfs_pass(qc, Hl, st["sig2"], M, Qk, np.zeros(M.shape[0]), st["P0"], lag_one=False)["f_smooth"]
    eps = np.where(obs, qc - g @ Hl.T, 0.0)
    w = eps.copy()
    for l in range(1, q + 1):                                        # the adjoint of the quasi-difference
        w[:ns - l] -= st["rho"][:, l - 1][None, :] * eps[l:]
    w = np.where(~np.isnan(new[q:]), w / st["sig2"][None, :], 0.0)
    if sd is not None:
        w = w * (sd[i_s] / np.asarray(sd))[None, :]
    return w


# ---------------------------------------------------------------------------------------------------- the entry's outputs
def expect(old, new, st, targets, v0=None, mean=None, sd=None):
    """One replicate; targets: (panel row t* >= q, series) pairs.  dict(yhat [3, G], news [T-q, N], weight [G, T-q, N], impact [G, N])."""
    T, N = new.shape
    q = st["rho"].shape[1]
    H = horizon(T, targets)
    rev = np.where(np.isnan(old), np.nan, new)
    par = [st[k] for k in KEYS]
    xh = [fe.expect(v, *par, H, v0=v0, mean=mean, sd=sd)["xhat"] for v in (old, rev, new)]
    yhat = np.array([[x[t - q, i] for t, i in targets] for x in xh])
    mu = np.zeros(N) if mean is None else np.asarray(mean, float)
    s = np.ones(N) if sd is None else np.asarray(sd, float)
    cells = (~np.isnan(new) & np.isnan(old))[q:]
    news = np.where(cells, (mu + s * new[q:]) - xh[1][:T - q], 0.0)
    weight = np.stack([weights(new, st, t - q, i, None if sd is None else s) for t, i in targets])
    return dict(yhat=yhat, news=news, weight=weight, impact=(weight * news[None]).sum(axis=1), cells=cells)


def joint(xfirst, st, n):
    """Mean [n N] and covariance of the n output rows given the first q panel rows, from the model's own recursion."""
    Lam, sig2, rho, Avar, Q, mu0, P0 = [st[k] for k in KEYS]
    N, r = Lam.shape
    q = rho.shape[1]
    p = Avar.shape[1] // r
    m = ao.state_lags(p, q)
    k = r * m
    dim = k + n * r + n * N

    def run(v):
        z = v[:k]
        eta = v[k:k + n * r].reshape(n, r)
        eps = v[k + n * r:].reshape(n, N)
        hist = [z[l * r:(l + 1) * r] for l in range(m)]
        eh = [xfirst[q - 1 - l] - Lam @ hist[l] for l in range(q)]
        xs = np.empty((n, N))
        for t in range(n):
            f = sum(Avar[:, l * r:(l + 1) * r] @ hist[l] for l in range(p)) + eta[t]
            e = sum(rho[:, l] * eh[l] for l in range(q)) + eps[t]
            xs[t] = Lam @ f + e
            hist = [f] + hist[:-1]
            eh = [e] + eh[:-1]
        return xs.ravel()

    mean_v = np.zeros(dim)
    mean_v[:k] = mu0
    S = np.zeros((dim, dim))
    S[:k, :k] = P0
    for t in range(n):
        S[k + t * r:k + (t + 1) * r, k + t * r:k + (t + 1) * r] = Q
    S[k + n * r:, k + n * r:] = np.diag(np.tile(sig2, n))
    x0 = run(np.zeros(dim))
    J = np.empty((n * N, dim))
    for j in range(dim):
        e = np.zeros(dim)
        e[j] = 1.0
        J[:, j] = run(e) - x0
    return x0 + J @ mean_v, J @ S @ J.T


def brute_force(old, new, st, targets):
    """Standardised units.  dict(yhat [3, G], weight [G, T-q, N] = Sigma^-1 c on the cells of new, news_weight [G, T-q, N] =
    Cov(y, I) Var(I)^-1 on the news cells (0 elsewhere), news [T-q, N], C (the joint covariance), n)."""
    T, N = new.shape
    q = st["rho"].shape[1]
    H = horizon(T, targets)
    n, ns = T + H - q, T - q
    rev = np.where(np.isnan(old), np.nan, new)
    pad = np.full((H, N), np.nan)

    def cond(v):
        mx, C = joint(v[:q], st, n)
        y = np.vstack([v[q:], pad]).ravel()
        o = ~np.isnan(y)
        full = mx + C[:, o] @ np.linalg.solve(C[np.ix_(o, o)], y[o] - mx[o])
        return np.where(o, y, full), C, o

    (xo, C, oo), (xr, _, _), (xn, _, on) = cond(old), cond(rev), cond(new)
    tidx = [(t - q) * N + i for t, i in targets]
    yhat = np.array([[x[j] for j in tidx] for x in (xo, xr, xn)])
    nw = on & ~oo
    news = np.where(nw, np.vstack([new[q:], pad]).ravel() - xr, 0.0)
    weight = np.zeros((len(tidx), n * N))
    news_weight = np.zeros((len(tidx), n * N))
    Coo_inv_Con = np.linalg.solve(C[np.ix_(oo, oo)], C[np.ix_(oo, nw)])
    VI = C[np.ix_(nw, nw)] - C[np.ix_(nw, oo)] @ Coo_inv_Con                    # Var(I) = Var(x_news | old)
    for g, j in enumerate(tidx):
        weight[g, on] = np.linalg.solve(C[np.ix_(on, on)], C[on, j])
        if nw.any():
            cyI = C[j, nw] - C[j, oo] @ Coo_inv_Con                             # Cov(y, I) = Cov(y, x_news | old)
            news_weight[g, nw] = np.linalg.solve(VI, cyI)
    sh = (len(tidx), n, N)
    return dict(yhat=yhat, weight=weight.reshape(sh)[:, :ns], news_weight=news_weight.reshape(sh)[:, :ns],
                news=news.reshape(n, N)[:ns], C=C, n=n)


def quasi_diff_of_cov(C, st, j, n):
    """D applied to the dense Cov(x, y_j): [n, N] (the first q panel rows are conditioning values: no covariance)."""
    N, q = st["rho"].shape
    c = C[:, j].reshape(n, N)
    out = c.copy()
    for l in range(1, q + 1):
        out[l:] -= st["rho"][:, l - 1][None, :] * c[:n - l]
    return out
