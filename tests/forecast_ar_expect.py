"""Expectation model of dfm_forecast_ar_batch (include/dfm_hip.h; csrc/forecast_ar.hip) on the CPU, three texts:

  expect        the oracle's AR pass (oracle.ar_oracle.kfs_pass_ar) over the panel with H all-missing rows appended, residuals of the
                observed cells, then PER SERIES dense Gaussian conditioning of e on its residuals (dense_idio: Cov(e) is built from
                v0, rho and sig2 and conditioned on the observed cells -- no recursion) and the header's cell formulas;
  two_filter    a NumPy restatement of the recursion the two kernels run (backward information message, forward filter, the message
                joined to the forward moments by rank-one updates), checked against dense_idio by tests/test_forecast_ar_cpu.py;
  brute_force   balanced panels only: the joint Gaussian of every cell, horizon included, from the model's OWN recursion (no
                quasi-differencing, no two-step argument), conditioned on rows q .. T-1 given rows 0 .. q-1: the exact conditional
                mean and variance of the horizon cells.

Shared by tests/test_forecast_ar_cpu.py and tests/test_gpu_forecast_ar.py; geometry() restates series_geometry of
csrc/dfm_cellgeom.h."""
import numpy as np

from oracle import ar_oracle as ao
from oracle import kalman_oracle as ko


# ---------------------------------------------------------------------------------------------------- the idiosyncratic smoother
PIVOT_TOL = 2.0 ** -44          # kFcArPivotTol of csrc/forecast_ar.hip

def idio_cov(n, rho, sig2, v0):
    """Cov of (e_0 .. e_{n-1}): e_t = sum_l rho_l e_{t-l} + eps_t, the q terms before row 0 ~ N(0, v0 I), eps ~ N(0, sig2)."""
    q = len(rho)
    G = np.zeros((n + q, n + q))                       # e_full = G (pre, eps); e_full[j] = e_{j-q}, pre in the order e_{-q} .. e_{-1}
    G[:q, :q] = np.eye(q)
    for t in range(n):
        G[q + t, q + t] = 1.0
        for l in range(1, q + 1):
            G[q + t] += rho[l - 1] * G[q + t - l]
    D = np.concatenate([np.full(q, v0), np.full(n, sig2)])
    C = (G * D) @ G.T
    return C[q:, q:]


def dense_idio(u, rho, sig2, v0):
    """u [n] (NaN = not observed) -> (ehat [n], V [n]): mean and variance of e_t given the observed entries of u, by conditioning
    the dense covariance.  Observed entries: u itself and exactly 0."""
    n = len(u)
    obs = ~np.isnan(u)
    C = idio_cov(n, rho, sig2, v0)
    eh = np.where(obs, u, 0.0)
    V = np.zeros(n)
    mis = ~obs
    if mis.any():
        if obs.any():
            Coo = C[np.ix_(obs, obs)]
            Cmo = C[np.ix_(mis, obs)]
            K = np.linalg.solve(Coo, Cmo.T).T
            eh[mis] = K @ u[obs]
            V[mis] = np.diag(C[np.ix_(mis, mis)] - K @ Cmo.T)
        else:
            V[mis] = np.diag(C)[mis]
    return eh, V


def two_filter(u, rho, sig2, v0):
    """The kernels' recursion for one series.  Returns (ehat, V, stored): stored = the rows whose backward message is kept (missing
    with a later observed cell)."""
    n, q = len(u), len(rho)
    obs = ~np.isnan(u)
    rho = np.asarray(rho, float)
    # backward: m_t(a_t) ~ exp(-a' Om a / 2 + eta' a) from the residuals after t, a_t = (e_t .. e_{t-q+1}).  Row t observed:
    # a_t = (u_t, a_{t-1}[:q-1]) and the density of u_t given a_{t-1} joins.  Row t missing: e_t = rho' a_{t-1} + eps is integrated
    # out, M = Om - Om e0 e0' Om / (Om_00 + 1 / sig2) and Om_{t-1} = F' M F with F = [rho'; I 0] -- a downdate and products, no
    # difference of large terms, so a message that has decayed to 1e-15 keeps its relative accuracy.
    Om, eta, seen = np.zeros((q, q)), np.zeros(q), False
    msg = {}
    for t in range(n - 1, -1, -1):
        if not obs[t] and seen:
            msg[t] = (Om.copy(), eta.copy())
        On, en = np.zeros((q, q)), np.zeros(q)
        if obs[t]:
            On[:q - 1, :q - 1] = Om[1:, 1:]
            en[:q - 1] = eta[1:] - Om[1:, 0] * u[t]
            On += np.outer(rho, rho) / sig2
            en += rho * (u[t] / sig2)
            seen = True
        elif seen:
            s = 1.0 / (Om[0, 0] + 1.0 / sig2)
            M = Om - np.outer(Om[:, 0], Om[0, :]) * s
            h = eta - Om[:, 0] * (eta[0] * s)
            MF = np.outer(M[:, 0], rho)
            MF[:, :q - 1] += M[:, 1:]
            On = np.outer(rho, MF[0])
            On[:q - 1] += MF[1:]
            On = np.tril(On) + np.tril(On, -1).T
            en = rho * h[0]
            en[:q - 1] += h[1:]
        Om, eta = On, en
    # forward: a_t | residuals up to t
    a, P = np.zeros(q), v0 * np.eye(q)
    eh, V = np.zeros(n), np.zeros(n)
    for t in range(n):
        rP = rho @ P
        Pn = np.empty((q, q))
        Pn[0, 0] = rP @ rho + sig2
        Pn[0, 1:] = rP[:q - 1]
        Pn[1:, 0] = rP[:q - 1]
        Pn[1:, 1:] = P[:q - 1, :q - 1]
        a = np.concatenate([[rho @ a], a[:q - 1]])
        P = Pn
        if obs[t]:
            k = P[:, 0] / P[0, 0]
            a = a + k * (u[t] - a[0])
            P = P - np.outer(k, P[0])
            a[0] = u[t]
            P[0, :] = 0.0
            P[:, 0] = 0.0
            eh[t], V[t] = u[t], 0.0
            continue
        am, Pm = a.copy(), P.copy()
        if t in msg:
            # Om = L D L' (unit lower L, D >= 0; a pivot not above PIVOT_TOL of its diagonal entry is rounding noise of a
            # rank-deficient message and drops its column), eta = L z: q pseudo-observations w_j' a with precision d_j, joined
            # one at a time -- every denominator is 1 + d_j w_j' P w_j >= 1
            Om, eta = msg[t]
            L, d = np.eye(q), np.zeros(q)
            for j in range(q):
                piv = Om[j, j] - sum(L[j, k] * L[j, k] * d[k] for k in range(j))
                ok = piv > PIVOT_TOL * Om[j, j]
                d[j] = piv if ok else 0.0
                inv = 1.0 / piv if ok else 0.0
                for i in range(j + 1, q):
                    L[i, j] = (Om[i, j] - sum(L[i, k] * L[j, k] * d[k] for k in range(j))) * inv
            z = np.zeros(q)
            for j in range(q):
                z[j] = eta[j] - sum(L[j, k] * z[k] for k in range(j))
            for j in range(q):
                w = L[:, j]
                Pw = Pm @ w
                den = 1.0 / (1.0 + d[j] * (w @ Pw))
                am = am + Pw * ((z[j] - d[j] * (w @ am)) * den)
                Pm = Pm - np.outer(Pw, Pw) * (d[j] * den)
        eh[t], V[t] = am[0], Pm[0, 0]
    return eh, V, sorted(msg)


# ---------------------------------------------------------------------------------------------------- the entry's outputs
def expect(x, Lam, sig2, rho, Avar, Q, mu0, P0, H, v0=None, mean=None, sd=None, idio=dense_idio):
    """One replicate: x [T, N] (NaN = missing), rho [N, q].  Returns dict(xhat, xvar, common, idio [n, N], f [n, r],
    P [n, r(r+1)/2] packed lower, loglik), n = T + H - q (panel rows q .. T + H - 1)."""
    T, N = x.shape
    r, q = Lam.shape[1], rho.shape[1]
    xp = np.vstack([x, np.full((H, N), np.nan)])
    out = ao.kfs_pass_ar(xp, Lam, sig2, rho, Avar, Q, mu0, P0)
    f = out["f_smooth"][:, :r]
    P = out["P_smooth"][:, :r, :r]
    xo = xp[q:]
    m = f @ Lam.T
    u = xo - m
    v0 = sig2 if v0 is None else np.asarray(v0, float)
    eh, V = np.empty_like(u), np.empty_like(u)
    for i in range(N):
        eh[:, i], V[:, i] = idio(u[:, i], rho[i], sig2[i], v0[i])[:2]
    mu = np.zeros(N) if mean is None else np.asarray(mean, float)
    s = np.ones(N) if sd is None else np.asarray(sd, float)
    obs = ~np.isnan(xo)
    quad = np.einsum("ij,tjk,ik->ti", Lam, P, Lam)
    common = m if mean is None else mu + s * m
    idio_out = np.where(obs, s * u, s * eh)
    xobs = xo if mean is None else mu + s * xo
    xhat = np.where(obs, xobs, common + idio_out)
    xvar = np.where(obs, 0.0, s * s * (quad + V))
    return dict(xhat=xhat, xvar=xvar, common=common, idio=idio_out, f=f, P=ko.pack_sym(P), loglik=out["loglik"])


def brute_force(x, Lam, sig2, rho, Avar, Q, mu0, P0, H):
    """Balanced x [T, N]: mean and variance [H, N] of the horizon cells given rows q .. T-1 (and the first q rows, on which the
    model conditions), from the joint Gaussian of (z_q, eta, eps) pushed through the model's own recursion."""
    T, N = x.shape
    r, q = Lam.shape[1], rho.shape[1]
    p = Avar.shape[1] // r
    m = ao.state_lags(p, q)
    k = r * m
    n = T + H - q
    dim = k + n * r + n * N

    def run(v):
        z = v[:k]
        eta = v[k:k + n * r].reshape(n, r)
        eps = v[k + n * r:].reshape(n, N)
        hist = [z[l * r:(l + 1) * r] for l in range(m)]
        eh = [x[q - 1 - l] - Lam @ hist[l] for l in range(q)]
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
    mx = x0 + J @ mean_v
    C = J @ S @ J.T
    no = (T - q) * N
    y = x[q:].ravel()
    K = np.linalg.solve(C[:no, :no], C[:no, no:]).T
    mean_h = mx[no:] + K @ (y - mx[:no])
    var_h = np.diag(C[no:, no:] - K @ C[:no, no:])
    return mean_h.reshape(H, N), var_h.reshape(H, N)


# ---------------------------------------------------------------------------------------------------- inputs
def synth(b, N, T, r, p, q, seed=ko.SEED0):
    """A seeded balanced panel with its start parameters (ao.synth_ar), rho rescaled so that sum_l |rho_il| <= 0.85, and a v0."""
    x, st = ao.synth_ar(b, N, T, r, p, q, seed=seed)
    rng = np.random.default_rng([seed, b, N, q, 11])
    rho = np.zeros((N, q))
    rho[:, 0] = rng.uniform(-0.3, 0.6, N)
    for l in range(1, q):
        rho[:, l] = rng.uniform(-0.25, 0.25, N) / l
    s = np.abs(rho).sum(axis=1)
    rho *= np.minimum(1.0, 0.85 / np.maximum(s, 1e-300))[:, None]
    st = dict(st, rho=rho, sig2=st["sig2"] * rng.uniform(0.6, 1.4, N))
    v0 = st["sig2"] * rng.uniform(0.5, 3.0, N)
    return x, st, v0


# ---------------------------------------------------------------------------------------------------- launch geometry
def geometry(N, row_doubles, rows, lds_bytes=48 * 1024, max_rows=32):
    """series_geometry of csrc/dfm_cellgeom.h: (NPB, G, RC, nchunk, nsblk, threads)."""
    nsblk = (N + 255) // 256
    NPB = (N + nsblk - 1) // nsblk
    threads = (NPB + 63) // 64 * 64
    rc = min(max_rows, lds_bytes // (row_doubles * 8), rows)
    rc = max(rc, 1)
    return NPB, 1, rc, (rows + rc - 1) // rc, nsblk, threads


# ---------------------------------------------------------------------------------------------------- the GPU case table
KEYS = ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")
N_KINDS = 10


def apply_pattern(x, q, first=0):
    """Missing cells by series: series i gets kind (i + first) % N_KINDS (rows are panel rows; output row 0 is panel row q).
    Panels too short for a kind leave that series balanced.  In place; returns the kinds used."""
    T, N = x.shape
    used = set()
    mid = q + (T - q) // 2
    for i in range(N):
        kind = (i + first) % N_KINDS
        col = x[:, i]
        if kind == 1 and q >= 2 and T - q > q:            # a ragged edge shorter than q
            col[T - (q - 1):] = np.nan
        elif kind == 2 and T - q > q + 3:                 # a ragged edge longer than q
            col[T - (q + 2):] = np.nan
        elif kind == 3 and T - q >= 5:                    # an isolated interior gap
            col[mid] = np.nan
        elif kind == 4 and T - q >= q + 5:                # a gap of q or more cells
            col[mid - 1:mid + q] = np.nan
        elif kind == 5 and T - q >= 8:                    # two gaps fewer than q apart (one observed cell between them)
            col[mid - 2:mid] = np.nan
            col[mid + 1] = np.nan
        elif kind == 6:                                   # a missing cell in output row 0
            col[q] = np.nan
        elif kind == 7:                                   # no observed cell at all
            col[:] = np.nan
        elif kind == 8:                                   # observed only in its last row
            col[:T - 1] = np.nan
        elif kind == 9 and T - q >= 4:                    # a missing cell among the first q rows and the output row after a gap at 0
            col[0] = np.nan
            col[q:q + 2] = np.nan
        else:
            continue
        used.add(kind)
    return used


# name -> B, N, T, r, p, q, H, first pattern kind (None: balanced)
CASES = {
    "q1_n1_gap": (1, 1, 40, 1, 1, 1, 1, 4),
    "q1_n1_none_observed": (1, 1, 12, 1, 1, 1, 2, 7),
    "q2_p_eq_n64_h0": (3, 64, 40, 2, 3, 2, 0, 0),
    "q3_r8_n65_long_h": (1, 65, 41, 8, 1, 3, 41, 3),
    "q4_p_gt_n139": (3, 139, 40, 1, 6, 4, 4, 1),
    "q1_n256_balanced": (1, 256, 40, 2, 1, 1, 1, None),
    "q1_n257_two_blocks": (1, 257, 40, 2, 2, 1, 2, 2),
    "q1_n513_three_blocks": (1, 513, 39, 2, 1, 1, 3, 5),
    "q2_t_min_h0": (1, 6, 3, 1, 1, 2, 0, 4),
    "q4_t_min_h1": (1, 12, 5, 2, 1, 4, 1, 0),
    "q3_balanced_h5": (1, 10, 24, 2, 2, 3, 5, None),
}


def make_case(name):
    """The inputs of a case: dict(dims, x [B,T,N], st (KEYS -> stacked arrays), v0, mean, sd [B,N], kinds)."""
    B, N, T, r, p, q, H, first = CASES[name]
    xs, sts, v0s = [], [], []
    kinds = set()
    for b in range(B):
        Ts = max(T, 3 * r + 12)                                      # the start's PCA wants a few rows; short panels are cut from it
        x, st, v0 = synth(b + 3, max(N, r + 2), Ts, r, p, q)
        x = np.ascontiguousarray(x[:T, :N])
        st = dict(st, Lam=st["Lam"][:N], sig2=st["sig2"][:N], rho=st["rho"][:N])
        if first is not None:
            kinds |= apply_pattern(x, q, first + b)
        xs.append(x); sts.append(st); v0s.append(v0[:N])
    rng = np.random.default_rng([5, N, T, q])
    return dict(dims=(B, N, T, r, p, q, H), x=np.stack(xs), st={k: np.stack([s[k] for s in sts]) for k in KEYS}, v0=np.stack(v0s),
                mean=rng.standard_normal((B, N)), sd=rng.uniform(0.5, 2.0, (B, N)), kinds=kinds)


def expect_case(c, b, v0=True, scaled=False):
    H = c["dims"][6]
    return expect(c["x"][b], *[c["st"][k][b] for k in KEYS], H, v0=c["v0"][b] if v0 else None,
                  mean=c["mean"][b] if scaled else None, sd=c["sd"][b] if scaled else None)
