"""Expectation model of dfm_simsmooth_batch (include/dfm_hip.h) on the CPU, in two parts:
  draw_from_normals  steps 1-6 of the header for given standard normals (the oracle's smoother pass for step 3)
  stream_normals     those normals from the header's stream table (oracle/synth_oracle.py's Philox4x32-10 and Box-Muller)
Shared by tests/test_simsmooth_cpu.py (checked against brute-force Gaussian conditioning) and tests/test_gpu_simsmooth.py."""
import numpy as np

from oracle import kalman_oracle as ko
from oracle import synth_oracle as so
from oracle import varp_oracle as vo

PSD_TOL = 1e-12


def psd_root(M):
    """Lower L with L L' = M: Cholesky on the lower triangle, a column whose pivot is <= PSD_TOL trace(M) is zero."""
    M = np.asarray(M, float)
    n = M.shape[0]
    tol = PSD_TOL * np.trace(M)
    L = np.zeros((n, n))
    for j in range(n):
        dj = M[j, j] - L[j, :j] @ L[j, :j]
        if dj <= tol:
            continue
        L[j, j] = np.sqrt(dj)
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def sizes(T, H, N, r, p):
    """Shapes of the normals of one draw: n0 [r p], eta [T+H, r], eps_plus [T, N], eps [T+H, N]."""
    return dict(n0=(r * p,), eta=(T + H, r), eps_plus=(T, N), eps=(T + H, N))


def _pairs(key, stream, nrow, ncol):
    h = (ncol + 1) // 2
    z0, z1 = so.normal2(key, stream, np.arange(nrow * h))
    z = np.empty((nrow, 2 * h))
    z[:, 0::2] = z0.reshape(nrow, h)
    z[:, 1::2] = z1.reshape(nrow, h)
    return z[:, :ncol]


def stream_normals(seed, first_draw, d, b, T, H, N, r, p):
    """The normals of draw d of replicate b (header stream table): key = replicate_key(seed, first_draw + d), word 16 b + s."""
    key = so.replicate_key(seed, first_draw + d)
    w = 16 * b
    return dict(n0=_pairs(key, w + 1, 1, r * p)[0], eta=_pairs(key, w + 2, T + H, r), eps_plus=_pairs(key, w + 3, T, N),
                eps=_pairs(key, w + 4, T + H, N))


def smoothed_mean(x, Lam, R, A, Q, mu0, P0, p):
    r = Lam.shape[1]
    if p == 1:
        out = ko.kfs_pass(x, Lam, R, A, Q, mu0, P0, lag_one=False)
    else:
        out = vo.kfs_pass_varp(x, Lam, R, A, Q, mu0, P0, p)
    return out["f_smooth"][:, :r]


def _recursion(A, LQ, eta, z, rows, f):
    """f[t] = A z + L_Q eta[t] for t in rows; z = (row t-1, .., row t-p) updated as it goes."""
    r = LQ.shape[0]
    for t in rows:
        v = A @ z + LQ @ eta[t]
        f[t] = v
        z = np.concatenate([v, z[:-r]])
    return z


def draw_from_normals(x, Lam, R, A, Q, mu0, P0, H, p, nz, mean=None, sd=None, roots=None):
    """One draw of one replicate: x [T, N] (NaN = missing), A = [A_1 .. A_p] (r, r p); nz = dict of normals (`sizes`).
    Returns (f [T+H, r], xd [T+H, N]) -- f_draw and x_draw of the header."""
    x = np.asarray(x, float)
    T, N = x.shape
    r = Lam.shape[1]
    k = r * p
    LP0, LQ = roots if roots is not None else (psd_root(P0), psd_root(Q))
    sR = np.sqrt(R)
    # 1. unconditional simulation
    fp = np.empty((T + H, r))
    z0 = mu0 + LP0 @ nz["n0"]
    _recursion(A, LQ, nz["eta"], z0, range(T), fp)
    xplus = fp[:T] @ Lam.T + sR * nz["eps_plus"]
    # 2. difference panel, 3. its smoothed mean with mu0 = 0
    Dp = np.where(np.isnan(x), np.nan, x - xplus)
    g = smoothed_mean(Dp, Lam, R, A, Q, np.zeros(k), P0, p)
    # 4. in sample, 5. the horizon
    f = np.empty((T + H, r))
    f[:T] = fp[:T] + g
    z = np.concatenate([f[T - 1 - j] for j in range(p)])
    _recursion(A, LQ, nz["eta"], z, range(T, T + H), f)
    # 6. cells
    xp = np.vstack([x, np.full((H, N), np.nan)])
    drawn = f @ Lam.T + sR * nz["eps"]
    xd = np.where(np.isnan(xp), drawn, xp)
    if mean is not None:
        xd = np.asarray(mean, float) + np.asarray(sd, float) * xd
    return f, xd


def draw(x, Lam, R, A, Q, mu0, P0, H, p, seed, first_draw, d, b, mean=None, sd=None):
    """draw_from_normals on the header's stream: what dfm_simsmooth_batch returns for (b, d)."""
    T, N = x.shape
    nz = stream_normals(seed, first_draw, d, b, T, H, N, Lam.shape[1], p)
    return draw_from_normals(x, Lam, R, A, Q, mu0, P0, H, p, nz, mean=mean, sd=sd)
