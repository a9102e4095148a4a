"""Expectation model of dfm_filter_ar_batch (include/dfm_hip.h) on the CPU, sharing nothing with csrc/filter_ar.hip: the textbook
Kalman filter on the quasi-differenced state space with the n_t x n_t innovation covariance of each row's observed cells (no
collapse, no root), the h-step forecasts of every origin by the model's own recursions (powers of the companion matrix, the AR(q)
recursion run forward), the three evaluation sums as plain loops over origins with the header's qualification rule.  Also the
restatement of the arguments launch_filter_ar_fill gives cell_geometry, the missing-pattern panel and the GPU case table.  Shared
by tests/test_filter_ar_cpu.py and tests/test_gpu_filter_ar.py."""
import numpy as np

from tests import forecast_ar_expect as fae
from tests import post_geometry as pg

LOG2PI = float(np.log(2.0 * np.pi))
KEYS = fae.KEYS                      # ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")
FTAR_MAX_THREADS = 512               # dfm_cellgeom.h kFtArFillMaxThreads
FTAR_LDS = 48 * 1024                 # dfm_cellgeom.h kFtArFillLds
OUTPUTS = ("z_pred", "P_pred", "z_filt", "P_filt", "loglik_t", "xpred", "verr", "vstd", "msfe", "msfe_common", "msfe0", "cnt")


def state_space(Lam, rho, Avar, Q):
    """(LamK [N, k], M [k, k], Qc [k, k], m): loadings [lam_i, -rho_i1 lam_i, .., -rho_iq lam_i, 0..] on z_t = (f_t .. f_{t-m+1})."""
    N, r = Lam.shape
    q = rho.shape[1]
    p = Avar.shape[1] // r
    m = max(p, q + 1)
    k = r * m
    Z = np.zeros((N, k))
    Z[:, :r] = Lam
    for l in range(1, q + 1):
        Z[:, l * r:(l + 1) * r] = -rho[:, l - 1:l] * Lam
    M = np.zeros((k, k))
    M[:r, :r * p] = Avar
    M[r:, :k - r] = np.eye(k - r)
    Qc = np.zeros((k, k))
    Qc[:r, :r] = Q
    return Z, M, Qc, m


def quasi_difference(x, rho):
    """y [T - q, N]: y_t = x_t - sum_l rho_l x_{t-l} for the panel rows t = q .. T-1; NaN when x_ti or one of its q lags is."""
    T = x.shape[0]
    q = rho.shape[1]
    y = x[q:].copy()
    for l in range(1, q + 1):
        y = y - rho[:, l - 1] * x[q - l:T - l]
    return y


def pack(P):
    il = np.tril_indices(P.shape[-1])
    return P[..., il[0], il[1]]


def textbook_filter(y, Z, R, M, Qc, mu0, P0):
    """z_pred, P_pred, z_filt, P_filt, ll_t over the rows of y."""
    n = y.shape[0]
    k = M.shape[0]
    zp = np.empty((n, k)); Pp = np.empty((n, k, k)); zf = np.empty((n, k)); Pf = np.empty((n, k, k)); ll = np.zeros(n)
    z, P = np.asarray(mu0, float), np.asarray(P0, float)
    P = np.tril(P) + np.tril(P, -1).T                  # (the entry reads the lower triangle)
    for t in range(n):
        z = M @ z
        P = M @ P @ M.T + Qc
        P = 0.5 * (P + P.T)
        zp[t], Pp[t] = z, P
        o = ~np.isnan(y[t])
        if o.any():
            Zt = Z[o]
            F = Zt @ P @ Zt.T + np.diag(R[o])
            v = y[t, o] - Zt @ z
            sol = np.linalg.solve(F, np.column_stack([Zt @ P, v]))
            K = sol[:, :k].T
            z = z + K @ v
            P = P - K @ Zt @ P
            P = 0.5 * (P + P.T)
            ll[t] = -0.5 * (o.sum() * LOG2PI + np.linalg.slogdet(F)[1] + v @ sol[:, k])
        zf[t], Pf[t] = z, P
    return zp, Pp, zf, Pf, ll


def forecasts(x, Lam, rho, M, zf_t, t, H):
    """The H forecasts made at origin t (a panel row >= q) from z_{t|t} = zf_t: (full [H, N], common [H, N], ok [N]).  ok: the cells
    t, t-1, .., t-q+1 of the series are all observed (NaN in `full` where not)."""
    N, r = Lam.shape
    q = rho.shape[1]
    hist = [x[t - l] - Lam @ zf_t[l * r:(l + 1) * r] for l in range(q)]        # e_{t-l|t}
    ok = ~np.isnan(np.stack(hist)).any(axis=0)
    full = np.empty((H, N)); common = np.empty((H, N))
    z = zf_t
    for h in range(H):
        z = M @ z
        e = sum(rho[:, l] * hist[l] for l in range(q))
        hist = [e] + hist[:-1]
        common[h] = Lam @ z[:r]
        full[h] = common[h] + e
    return full, common, ok


def expect(x, Lam, sig2, rho, Avar, Q, mu0, P0, H=0, t0=None, mean=None, sd=None):
    """Every output of dfm_filter_ar_batch for one replicate, in the entry's layouts (n = T - q rows, packed covariances)."""
    x = np.asarray(x, float)
    T, N = x.shape
    r, q = Lam.shape[1], rho.shape[1]
    t0 = q if t0 is None else t0
    Z, M, Qc, _ = state_space(Lam, rho, Avar, Q)
    w = r * (q + 1)
    y = quasi_difference(x, rho)
    zp, Pp, zf, Pf, ll = textbook_filter(y, Z, sig2, M, Qc, mu0, P0)
    mu = np.zeros(N) if mean is None else np.asarray(mean, float)
    s = np.ones(N) if sd is None else np.asarray(sd, float)
    mk = zp @ Z.T
    lagsum = sum(rho[:, l - 1] * x[q - l:T - l] for l in range(1, q + 1))      # NaN where a lag is missing
    var = np.einsum("ia,tab,ib->ti", Z[:, :w], Pp[:, :w, :w], Z[:, :w]) + sig2
    out = dict(z_pred=zp, P_pred=pack(Pp), z_filt=zf, P_filt=pack(Pf), loglik_t=ll, xpred=mu + s * (mk + lagsum), verr=s * (y - mk),
               vstd=(y - mk) / np.sqrt(var))
    if H > 0:
        e2 = np.zeros((H, N)); c2 = np.zeros((H, N)); x2 = np.zeros((H, N)); cnt = np.zeros((H, N), np.int32)
        for t in range(t0, T - 1):                       # origins in their order; horizon h has the origins t0 .. T-1-h
            full, common, ok = forecasts(x, Lam, rho, M, zf[t - q], t, min(H, T - 1 - t))
            for h in range(1, min(H, T - 1 - t) + 1):
                xv = x[t + h]
                for i in range(N):
                    if ok[i] and not np.isnan(xv[i]):
                        e2[h - 1, i] += (xv[i] - full[h - 1, i]) ** 2
                        c2[h - 1, i] += (xv[i] - common[h - 1, i]) ** 2
                        x2[h - 1, i] += xv[i] * xv[i]
                        cnt[h - 1, i] += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            nn = np.where(cnt > 0, cnt, np.nan)
            out.update(msfe=s * s * e2 / nn, msfe_common=s * s * c2 / nn, msfe0=s * s * x2 / nn, cnt=cnt)
    return out


# ---------------------------------------------------------------------------------------------------- the fill's launch geometry
def w_bucket(w):
    return 4 if w <= 4 else 8 if w <= 8 else 16 if w <= 16 else 32


def fill_row_doubles(r, q):
    """A staged row of filter_ar_fill_kernel: z_pred[:w] and the packed leading w x w block of P_pred, w = r (q + 1)."""
    w = r * (q + 1)
    return w + w * (w + 1) // 2


def fill_launch(B, N, r, q, T, aligned=True):
    """launch_filter_ar_fill (filter_ar.hip): SP = 2 for even N in a register bucket (of w) <= 16 with 16-byte aligned pointers;
    filter_ar_fill_kernel<WB, SP> over the T - q rows."""
    wb = w_bucket(r * (q + 1))
    sp = 2 if N % 2 == 0 and wb <= 16 and aligned else 1
    call = ((N + sp - 1) // sp, fill_row_doubles(r, q), T - q, FTAR_MAX_THREADS, FTAR_LDS)
    return pg._summary("filter_ar_fill_kernel", call, lambda g: (B * g["nchunk"] * g["nsblk"], 1, 1), SP=sp, WB=wb, vec=sp == 2)


# ---------------------------------------------------------------------------------------------------- inputs
def params_for(B, N, T, r, p, q, missing=0.0, first=0):
    """Panels [B, T, N] and parameters (KEYS -> stacked arrays) of a case: forecast_ar_expect.synth's seeded balanced panels with
    their start parameters, cut to T rows and N series, then cells dropped at rate `missing` (own seeded stream)."""
    xs, sts = [], []
    for b in range(B):
        x, st, _ = fae.synth(b + first + 3, max(N, r + 2), max(T, 3 * r + 12), r, p, q)
        x = np.ascontiguousarray(x[:T, :N])
        st = dict(st, Lam=st["Lam"][:N], sig2=st["sig2"][:N], rho=st["rho"][:N])
        if missing > 0.0:
            g = np.random.default_rng([17, b, N, T, q])
            x[g.random((T, N)) < missing] = np.nan
        xs.append(x); sts.append(st)
    return np.stack(xs), {k: np.ascontiguousarray(np.stack([np.asarray(s[k], float) for s in sts])) for k in KEYS}


def scales(B, N, scaled):
    if not scaled:
        return None, None
    g = np.random.default_rng([3, N])
    return g.standard_normal((B, N)), g.uniform(0.5, 3.0, (B, N))


def missing_pattern(x, q):
    """In place, on a panel [B, T, N] with T >= 6 q + 16 and N >= 8: an isolated gap, a gap of q + 1, a ragged edge, a row with no
    observed cell, a series never observed and a missing cell in panel row 0."""
    T = x.shape[1]
    x[:, q + 4, 0] = np.nan                              # an isolated gap
    x[:, 2 * q + 7:3 * q + 8, 1] = np.nan                # a gap of q + 1 cells
    x[:, T - 3:, 2] = np.nan                             # a ragged edge
    x[:, T - 1:, 3] = np.nan
    x[:, 4 * q + 10, :] = np.nan                         # a row with no observed cell
    x[:, :, 4] = np.nan                                  # a series never observed
    x[:, 0, 5] = np.nan                                  # a missing cell in panel row 0
    return x


# ---------------------------------------------------------------------------------------------------- the GPU case table
# (name, B, N, T, r, p, q, H, t0 (None: q), missing, scaled, aligned)
CASES = [
    ("q1_p_below_n64",        2, 64,  30, 2, 1, 1, 3,  5,    0.1,  True,  True),     # p < q + 1
    ("q1_p_at_n65",           2, 65,  30, 3, 2, 1, 3,  None, 0.1,  True,  True),     # p = q + 1, odd N
    ("q2_p_above_n139",       2, 139, 30, 2, 4, 2, 4,  10,   0.1,  True,  True),     # p > q + 1, k = 8 > w = 6
    ("q3_r1_n1",              2, 1,   30, 1, 2, 3, 3,  12,   0.05, False, True),     # r = 1, N = 1
    ("q4_r1_p6_n24",          2, 24,  40, 1, 6, 4, 3,  20,   0.04, True,  True),     # q = 4, p above
    ("q1_r8_p4_k32_w16",      2, 40,  24, 8, 4, 1, 2,  12,   0.1,  True,  True),     # w < k at the cap
    ("q3_r8_k32_w32",         2, 40,  24, 8, 2, 3, 2,  12,   0.04, False, True),     # w = k = 32
    ("q1_n256",               2, 256, 14, 2, 1, 1, 2,  6,    0.0,  True,  True),
    ("q1_n257_two_blocks",    2, 257, 14, 2, 2, 1, 2,  6,    0.1,  True,  True),
    ("q1_n513_three_blocks",  2, 513, 12, 2, 1, 1, 2,  5,    0.1,  False, True),
    ("q2_t_min",              2, 24,  3,  2, 1, 2, 2,  2,    0.0,  True,  True),     # T = q + 1: one row, no origin
    ("q2_long_span",          2, 24,  100, 2, 2, 2, 3, 20,   0.1,  True,  True),     # T - t0 > 64: two evaluation chunks
    ("q2_h0",                 2, 24,  20, 2, 2, 2, 0,  None, 0.0,  True,  True),
    ("q2_h1",                 2, 24,  20, 2, 2, 2, 1,  10,   0.1,  False, True),
    ("q2_h_beyond",           2, 24,  20, 2, 2, 2, 9,  14,   0.0,  True,  True),     # H >= T - t0: horizons without an origin
    ("q2_b1",                 1, 24,  20, 2, 2, 2, 2,  8,    0.1,  True,  True),
    ("q2_b3",                 3, 24,  20, 2, 2, 2, 2,  8,    0.1,  True,  True),
    ("q2_n130_misaligned",    2, 130, 20, 2, 2, 2, 2,  8,    0.1,  True,  False),    # outputs 8 bytes past a 16-byte boundary
    ("q1_r8_p4_misaligned",   2, 40,  16, 8, 4, 1, 2,  8,    0.0,  False, False),
]
CASE_KEYS = ("name", "B", "N", "T", "r", "p", "q", "H", "t0", "missing", "scaled", "aligned")


def case_dict(row):
    c = dict(zip(CASE_KEYS, row))
    if c["t0"] is None:
        c["t0"] = c["q"]
    return c


def make_case(row):
    """(case dict, x [B, T, N], st, mean, sd)."""
    c = case_dict(row)
    x, st = params_for(c["B"], c["N"], c["T"], c["r"], c["p"], c["q"], missing=c["missing"])
    mean, sd = scales(c["B"], c["N"], c["scaled"])
    return c, x, st, mean, sd


def expect_case(x, st, b, H, t0, mean, sd):
    return expect(x[b], *[st[k][b] for k in KEYS], H=H, t0=t0, mean=None if mean is None else mean[b],
                  sd=None if sd is None else sd[b])
