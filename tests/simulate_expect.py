"""Expectation model of dfm_simulate_batch and dfm_simulate_ar_batch (include/dfm_hip.h; csrc/simulate.hip) on the CPU: the contract
in NumPy, from the texts of tests/simsmooth_expect.py and tests/simsmooth_ar_expect.py (stream_normals, psd_root, the recursions).

  simulate        x_sim, f_sim of one (b, d) of dfm_simulate_batch: step 1 of simsmooth_expect.draw_from_normals, written out
  simulate_ar     x_sim, f_sim of one (b, d) of dfm_simulate_ar_batch: steps 1-4 of simsmooth_ar_expect.draw_from_normals with H = 0
  implied_cov     the covariance of the stacked panel the MODEL implies, from its companion form alone (no normals, no roots):
                  tests/test_simulate_cpu.py holds the sample covariance of the two functions above against it
  plain_launch / ar_launch   the launch geometry of the two kernels, restated from post_geometry.cell_geometry and
                  forecast_ar_expect.geometry

The mask.  A cell of x_sim is NaN exactly where the mask panel (plain) or the panel (AR, rows >= q) is NaN; no index of a normal
depends on it.  Rows < q of the AR form: with a panel they ARE the panel's rows, bit for bit (NaN stays NaN) -- the draw is
conditional on them; with no panel row q - l is lam_i' f+_{q-l} + sqrt(v0_i) n, f+_{q-l} being lag block l - 1 of z+ and n the
pre-sample normal l of stream 5 -- the very term the recursion starts from."""
import numpy as np

from oracle import ar_oracle as ao
from tests import forecast_ar_expect as fe
from tests import post_geometry as pg
from tests import simsmooth_ar_expect as sae
from tests import simsmooth_expect as sse

SIM_MAX_THREADS = 512                # simulate.hip kSimMaxThreads
SIM_LDS = 32 * 1024                  # simulate.hip kSimLds
SIMAR_LDS = 48 * 1024                # simulate.hip kSimArLds
SSAR_TAIL = 64                       # dfm_fcar.h kSsArLdsTail
SLICE = 8192                         # capi.hip kSsSlice: pass replicates per launch


def simulate(Lam, R, A, Q, mu0, P0, T, seed, first_draw, d, b, mask=None):
    """(x_sim [T, N], f_sim [T, r]) of draw d of replicate b; A = [A_1 .. A_p] (r, r p); mask [T, N] or None."""
    N, r = Lam.shape
    p = A.shape[1] // r
    nz = sse.stream_normals(seed, first_draw, d, b, T, 0, N, r, p)
    LP0, LQ = sse.psd_root(P0), sse.psd_root(Q)
    fp = np.empty((T, r))
    sse._recursion(A, LQ, nz["eta"], mu0 + LP0 @ nz["n0"], range(T), fp)
    x = fp @ Lam.T + np.sqrt(R) * nz["eps_plus"]
    if mask is not None:
        x[np.isnan(mask)] = np.nan
    return x, fp


def simulate_ar(Lam, sig2, rho, Avar, Q, mu0, P0, T, seed, first_draw, d, b, panel=None, v0=None):
    """(x_sim [T, N], f_sim [T - q, r]) of draw d of replicate b; rho [N, q]; panel [T, N] or None; v0 [N] or None (sig2)."""
    N, r = Lam.shape
    q = rho.shape[1]
    p = Avar.shape[1] // r
    m = ao.state_lags(p, q)
    n = T - q
    nz = sae.stream_normals(seed, first_draw, d, b, T, 0, N, r, p, q)
    v0 = sig2 if v0 is None else np.asarray(v0, float)
    LP0, LQ = sse.psd_root(P0), sse.psd_root(Q)
    X = np.full((T, N), np.nan) if panel is None else np.asarray(panel, float)
    z = mu0 + LP0 @ nz["n0"]
    hist = [z[l * r:(l + 1) * r] for l in range(m)]                      # f+_{q-1} .. f+_{q-m}
    eh = [np.where(np.isnan(X[q - l]), np.sqrt(v0) * nz["pre"][l - 1], X[q - l] - Lam @ hist[l - 1]) for l in range(1, q + 1)]
    x = np.empty((T, N))
    for l in range(1, q + 1):                                            # rows < q
        x[q - l] = X[q - l] if panel is not None else Lam @ hist[l - 1] + eh[l - 1]
    fp = np.empty((n, r))
    for t in range(n):
        f = sum(Avar[:, l * r:(l + 1) * r] @ hist[l] for l in range(p)) + LQ @ nz["eta"][t]
        e = sum(rho[:, l] * eh[l] for l in range(q)) + np.sqrt(sig2) * nz["eps_plus"][t]
        fp[t] = f
        x[q + t] = Lam @ f + e
        hist = [f] + hist[:-1]
        eh = [e] + eh[:-1]
    if panel is not None:
        x[q:][np.isnan(X[q:])] = np.nan
    return x, fp


# ------------------------------------------------------------------------------------------------- what the model implies
def _stack_cov(V0, F, Qs, obs):
    """Cov of the stacked observations y_j = C_j s_{tau_j} of the chain s_t = F s_{t-1} + w_t, Var(w) = Qs, Var(s_0) = V0;
    obs = [(tau_j, C_j)] with tau ascending from 0."""
    V = [V0]
    for _ in range(max(t for t, _ in obs)):
        V.append(F @ V[-1] @ F.T + Qs)
    rows = []
    for ta, Ca in obs:
        row = []
        for tb, Cb in obs:
            if ta <= tb:
                row.append(Ca @ V[ta] @ np.linalg.matrix_power(F, tb - ta).T @ Cb.T)
            else:
                row.append((Cb @ V[tb] @ np.linalg.matrix_power(F, ta - tb).T @ Ca.T).T)
        rows.append(row)
    return np.block(rows)


def implied_cov(Lam, R, A, Q, P0, T):
    """Cov(vec x_0 .. x_{T-1}) [T N, T N] of x_t = Lam f_t + e_t from the companion form: z_t = F z_{t-1} + (eta_t, 0), z_{-1} ~
    (mu0, P0), Var e = diag R."""
    N, r = Lam.shape
    k = A.shape[1]
    F = np.zeros((k, k)); F[:r] = A; F[r:, :k - r] = np.eye(k - r)
    Qs = np.zeros((k, k)); Qs[:r, :r] = Q
    C = np.hstack([Lam, np.zeros((N, k - r))])
    S = _stack_cov(P0, F, Qs, [(t + 1, C) for t in range(T)])
    return S + np.kron(np.eye(T), np.diag(R))


def implied_cov_ar(Lam, sig2, rho, Avar, Q, P0, v0, T):
    """The same for the AR form without a panel: the state (f_t .. f_{t-m+1}, e_t .. e_{t-q+1}) at panel row t, started at row
    q - 1 from blockdiag(P0, v0 on every lag); rows < q - 1 read the lags of that first state."""
    N, r = Lam.shape
    q = rho.shape[1]
    p = Avar.shape[1] // r
    m = ao.state_lags(p, q)
    k, ke = r * m, N * q
    F = np.zeros((k + ke, k + ke))
    F[:r, :r * p] = Avar
    F[r:k, :k - r] = np.eye(k - r)
    for l in range(q):
        F[k:k + N, k + l * N:k + (l + 1) * N] = np.diag(rho[:, l])
    F[k + N:, k:k + ke - N] = np.eye(ke - N)
    Qs = np.zeros_like(F); Qs[:r, :r] = Q; Qs[k:k + N, k:k + N] = np.diag(sig2)
    V0 = np.zeros_like(F); V0[:k, :k] = P0; V0[k:, k:] = np.kron(np.eye(q), np.diag(v0))

    def C(l):                                                            # x of lag l of the state: lam' f_{t-l} + e_{t-l}
        M = np.zeros((N, k + ke))
        M[:, l * r:(l + 1) * r] = Lam
        M[:, k + l * N:k + (l + 1) * N] = np.eye(N)
        return M
    obs = [(0, C(q - 1 - t)) for t in range(q)] + [(t - q + 1, C(0)) for t in range(q, T)]
    return _stack_cov(V0, F, Qs, obs)


# ------------------------------------------------------------------------------------------------- launch geometry
def plain_launch(B, D, N, r, T):
    """simulate.hip launch_simulate_cells: column pairs, r doubles per staged row, T rows; grid (pass replicates of the slice,
    nchunk, nsblk); the 16-byte path where N is even (the entries' arrays are 256-byte aligned)."""
    call = ((N + 1) // 2, r, T, SIM_MAX_THREADS, SIM_LDS)
    return pg._summary("simulate_cells_kernel", call, lambda g: (min(B * D, SLICE), g["nchunk"], g["nsblk"]), RB=pg.rb_bucket(r),
                       vec=N % 2 == 0)


def ar_launch(B, D, N, r, q, T):
    """simulate.hip launch_simar_q: series_geometry of N series, r doubles per staged row, T - q rows under the LDS left by the
    tail; min(B D, SLICE) nsblk workgroups; `paired`: SsArIdio's branch of each series block."""
    n, lds = T - q, SIMAR_LDS - 8 * SSAR_TAIL
    NPB, G, rc, nchunk, nsblk, threads = fe.geometry(N, r, n, lds_bytes=lds)
    return dict(kernel="simulate_ar_cells_kernel", Q=q, RB=4 if r <= 4 else 8 if r <= 8 else 16, NPB=NPB, G=G, RC=rc, nchunk=nchunk,
                nsblk=nsblk, threads=threads, n=n, call=(N, r, n, lds), grid=(min(B * D, SLICE) * nsblk, 1, 1),
                paired=tuple((s * NPB) % 2 == 0 for s in range(nsblk)))
