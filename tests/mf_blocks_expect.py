"""NumPy model of the mixed-frequency EM with FIXED loadings (include/dfm_hip.h: dfm_em_mf_blocks_batch), test infrastructure only.
The model, its pass and its transition step are tests/mf_expect.py's; `free` [N][r] (nonzero = estimated) restricts the series step:
with F the free and X the fixed coordinates of series i and k_i = |F|,

    lam_F = G_FF^-1 (b_F - G_FX lam_X),      R_i = (sum x^2 - 2 lam' b + lam' G lam) / n_i   (the whole lam),

a fixed loading keeps the value it has on entry; n_i < k_i + 1 or a G_FF that is not positive definite keeps lam_i and R_i;
k_i = 0 and n_i >= 1 updates R_i only.  Also the block-wise start of api.estimate_mixed_frequency(blocks=) and the case builder of
tests/test_gpu_mf_blocks.py."""
from __future__ import annotations

import numpy as np

from oracle import kalman_oracle as ko
from tests import mf_expect as me

KEYS = ("Lam", "R", "Avar", "Q", "mu0", "P0")


def series_moments(x, W, out, r, L):
    """Per series (n_i, G_i, b_i, sum x^2) from a pass's dict, as em_step_mf forms them."""
    T, N = x.shape
    zs, Ps = out["f_smooth"], out["P_smooth"]
    m = zs.shape[1] // r
    Ez = zs[:, :, None] * zs[:, None, :] + Ps
    zb = zs.reshape(T, m, r)[:, :L]
    Eb = Ez.reshape(T, m, r, m, r)[:, :L, :, :L, :]
    obs = ~np.isnan(x)
    res = []
    for i in range(N):
        o = obs[:, i]
        w = W[i]
        G = np.einsum("l,tlcmd,m->cd", w, Eb[o], w)
        b = np.einsum("l,tlc->tc", w, zb[o]).T @ x[o, i]
        res.append((int(o.sum()), G, b, (x[o, i] ** 2).sum()))
    return res


def em_step_mf_blocks(x, Lam, R, W, free, Avar, Q, mu0, P0):
    """One EM iteration; returns (new parameters, log-likelihood at the entering parameters, the pass's dict)."""
    x = np.asarray(x, float)
    free = np.asarray(free) != 0
    r = Lam.shape[1]
    new, ll, out = me.em_step_mf(x, Lam, R, W, Avar, Q, mu0, P0)      # the pass and the transition step; the series step is redone
    Lam_new = Lam.copy(); R_new = R.copy()
    for i, (n, G, b, sxx) in enumerate(series_moments(x, W, out, r, W.shape[1])):
        F = np.nonzero(free[i])[0]
        X = np.nonzero(~free[i])[0]
        if n < len(F) + 1:
            continue
        lam = Lam[i].copy()
        if len(F):
            GFF = G[np.ix_(F, F)]
            try:
                np.linalg.cholesky(GFF)
            except np.linalg.LinAlgError:
                continue
            rhs = b[F] - G[np.ix_(F, X)] @ lam[X] if len(X) else b[F]
            lam[F] = np.linalg.solve(GFF, rhs)
        Lam_new[i] = lam
        R_new[i] = (sxx - 2.0 * lam @ b + lam @ G @ lam) / n
    new = dict(new, Lam=Lam_new, R=R_new)
    return new, ll, out


def em_mf_blocks(x, params, W, free, max_iter=10, tol=0.0):
    """EM loop with mf_expect.em_mf's bookkeeping."""
    cur = {k: np.array(v, float) for k, v in params.items()}
    path = []
    out = None
    for it in range(max_iter):
        new, ll, out = em_step_mf_blocks(x, W=W, free=free, **cur)
        path.append(ll)
        if it >= 1 and tol > 0.0:
            if (path[-1] - path[-2]) / (0.5 * (abs(path[-1]) + abs(path[-2]))) < tol:
                break
        cur = new
    return cur, np.array(path), out


def blocks_free(membership, factors):
    """free [N][sum(factors)] of a block structure: block g's factors[g] columns are free on its member series."""
    membership = np.asarray(membership, bool)
    return np.concatenate([np.repeat(membership[:, g:g + 1], f, axis=1) for g, f in enumerate(factors)], axis=1)


def column_runs(free):
    """Maximal runs of equal adjacent columns of free: [(first column, one past the last, member series)]."""
    free = np.asarray(free) != 0
    runs, c0 = [], 0
    for c in range(1, free.shape[1] + 1):
        if c == free.shape[1] or not np.array_equal(free[:, c], free[:, c0]):
            runs.append((c0, c, free[:, c0]))
            c0 = c
    return runs


def mf_blocks_start(x, W, free, p):
    """The block-wise start: for each run of equal columns of `free`, in order, the first principal components of its fully observed
    monthly member series after the earlier runs' factors are projected out; every series regresses on its free aggregated factors
    only (fixed loadings start at 0); VAR(p), P0 and the variance floor as mf_expect.mf_start."""
    free = np.asarray(free) != 0
    T, N = x.shape
    r = free.shape[1]
    L = W.shape[1]
    m = max(p, L)
    monthly = (W[:, 0] == 1.0) & np.all(W[:, 1:] == 0.0, axis=1)
    full = ~np.isnan(x).any(axis=0)
    F = np.zeros((T, 0))
    for c0, c1, member in column_runs(free):
        sel = monthly & full & member
        assert sel.sum() >= c1 - c0
        xb = x[:, sel]
        if F.shape[1]:
            xb = xb - F @ np.linalg.lstsq(F, xb, rcond=None)[0]
        F = np.hstack([F, ko.pca_init(xb, c1 - c0)[1]])
    Lam = np.zeros((N, r)); R = np.ones(N)
    for i in range(N):
        fr = np.nonzero(free[i])[0]
        g = sum(W[i, l] * np.vstack([np.zeros((l, r)), F[:T - l]]) for l in range(L))[:, fr]
        o = ~np.isnan(x[:, i]); o[:L - 1] = False
        if o.sum() < len(fr) + 1:
            continue
        lam = np.linalg.lstsq(g[o], x[o, i], rcond=None)[0] if len(fr) else np.zeros(0)
        Lam[i, fr] = lam
        R[i] = max(np.mean((x[o, i] - g[o] @ lam) ** 2), 0.05)
    Z = np.hstack([F[p - 1 - l:T - l] for l in range(p)])
    Y, Xl = F[p:], Z[:-1]
    Avar = np.linalg.solve(Xl.T @ Xl, Xl.T @ Y).T
    e = Y - Xl @ Avar.T
    Q = e.T @ e / (T - p); Q = 0.5 * (Q + Q.T)
    Zm = np.hstack([F[m - 1 - l:T - l] for l in range(m)])
    P0 = Zm.T @ Zm / Zm.shape[0] + 1e-3 * np.eye(r * m)
    return dict(Lam=Lam, R=R, Avar=Avar, Q=Q, mu0=np.zeros(r * m), P0=0.5 * (P0 + P0.T))


def case_mask(N, r):
    """The mask of a test case: column 0 free everywhere, column c >= 1 free on the series with i mod (r - 1) == c - 1 (r = 1: free
    and fixed alternate), row 1 all fixed, and the loading (0, 0) fixed (build_case sets it to 1)."""
    i = np.arange(N)
    free = np.zeros((N, r), bool)
    free[:, 0] = True if r > 1 else (i % 2 == 0)
    for c in range(1, r):
        free[:, c] = i % (r - 1) == c - 1
    free[1] = False
    free[0, 0] = False
    return free


def thin_to(x, i, n):
    """Series i of every replicate keeps its first n cells that are observed in all replicates."""
    keep = np.nonzero(~np.isnan(x[:, :, i]).any(axis=0))[0][:n]
    assert len(keep) == n
    col = x[:, :, i].copy()
    x[:, :, i] = np.nan
    x[:, keep, i] = col[:, keep]


def build_case(B, Nm, Nq, T, r, p, kind="q_flow", missing=0.0, interleave=False):
    """B panels on mf_expect.synth_mf with one weight matrix and one mask (case_mask), the start with its fixed entries set -- zeros,
    and a 1 at (0, 0) -- and two thinned series: `at` with n_i = k_i observed cells (keeps its loadings) and `above` with n_i = k_i + 1
    and k_i < r (updates; the rule of the unrestricted model, n_i < r + 1, would have kept it).
    Returns (x [B,T,N], W, free, start dict of [B, ..], dict(at, above, fixed_row, one))."""
    xs, Ws, sts = zip(*[me.synth_mf(b, Nm, Nq, T, r, p, kind, missing=missing, interleave=interleave) for b in range(B)])
    if interleave:                                             # one order for the batch: replicate 0's
        assert all(np.array_equal(np.sort(W, axis=0), np.sort(Ws[0], axis=0)) for W in Ws)
        xs = list(xs)
        for b in range(1, B):
            order = _match_rows(Ws[b], Ws[0])
            xs[b] = xs[b][:, order]
            sts[b]["Lam"], sts[b]["R"] = sts[b]["Lam"][order], sts[b]["R"][order]
    else:
        assert all(np.array_equal(W, Ws[0]) for W in Ws)
    W = Ws[0]
    x = np.stack(xs)
    N = Nm + Nq
    free = case_mask(N, r)
    monthly = np.nonzero((W[:, 0] == 1.0) & np.all(W[:, 1:] == 0.0, axis=1))[0]
    k = free.sum(1)
    cand = [i for i in monthly if i > 1 and k[i] >= 1]
    cand = [i for i in cand if k[i] < r] or cand                # (r <= 2: every such series has k_i = r)
    at, above = cand[0], cand[1]
    thin_to(x, at, k[at])
    thin_to(x, above, k[above] + 1)
    st = {key: np.stack([s[key] for s in sts]) for key in KEYS}
    st["Lam"] = np.where(free[None], st["Lam"], 0.0)
    st["Lam"][:, 0, 0] = 1.0
    return x, W, free, st, dict(at=int(at), above=int(above), fixed_row=1, one=(0, 0))


def _match_rows(Wb, W0):
    """A permutation `order` with Wb[order] == W0 (rows are weight patterns; equal rows are matched in order)."""
    order, used = [], np.zeros(len(Wb), bool)
    for w in W0:
        j = next(j for j in range(len(Wb)) if not used[j] and np.array_equal(Wb[j], w))
        used[j] = True
        order.append(j)
    return np.array(order)
