"""Expectation model of dfm_filter_batch (include/dfm_hip.h) on the CPU, sharing nothing with csrc/filter.hip: the textbook Kalman
filter on the companion state with the n_t x n_t innovation covariance of each row's observed cells (no collapse), h-step
predictions by powers of the companion matrix, the evaluation sums as plain loops.  Also the Python restatements the CPU tests
hold against it: the collapsed update filter_kernel writes, and the arguments launch_filter_fill gives cell_geometry.  Shared by
tests/test_filter_cpu.py and tests/test_gpu_filter.py."""
import numpy as np

from tests import post_geometry as pg
from tests.simsmooth_expect import psd_root      # lower root with the zero-column rule: a pivot <= 1e-12 trace gives a zero column
from tests.structural_expect import KEYS, synth  # noqa: F401  (the oracle's synthetic panels and parameters)

LOG2PI = float(np.log(2.0 * np.pi))
FT_MAX_THREADS = 512                 # dfm_filter.h kFtFillMaxThreads
FT_LDS = 48 * 1024                   # dfm_filter.h kFtFillLds


def companion(A, Q):
    r, k = A.shape
    M = np.zeros((k, k))
    M[:r] = A
    M[r:, :k - r] = np.eye(k - r)
    Qc = np.zeros((k, k))
    Qc[:r, :r] = Q
    return M, Qc


def pack(P):
    il = np.tril_indices(P.shape[-1])
    return P[..., il[0], il[1]]


def textbook_filter(x, Lam, R, A, Q, mu0, P0):
    """z_pred, P_pred, z_filt, P_filt, ll_t of one replicate.  A = [A_1 .. A_p] (r x r p)."""
    x = np.asarray(x, float)
    T, N = x.shape
    r, k = A.shape
    M, Qc = companion(A, Q)
    Z = np.zeros((N, k))
    Z[:, :r] = Lam
    zp = np.empty((T, k)); Pp = np.empty((T, k, k)); zf = np.empty((T, k)); Pf = np.empty((T, k, k)); ll = np.zeros(T)
    z, P = np.asarray(mu0, float), np.asarray(P0, float)
    for t in range(T):
        z = M @ z
        P = M @ P @ M.T + Qc
        P = 0.5 * (P + P.T)
        zp[t], Pp[t] = z, P
        w = ~np.isnan(x[t])
        if w.any():
            Zt = Z[w]
            F = Zt @ P @ Zt.T + np.diag(R[w])
            v = x[t, w] - Zt @ z
            K = np.linalg.solve(F, Zt @ P).T
            z = z + K @ v
            P = P - K @ Zt @ P
            P = 0.5 * (P + P.T)
            ll[t] = -0.5 * (w.sum() * LOG2PI + np.linalg.slogdet(F)[1] + v @ np.linalg.solve(F, v))
        zf[t], Pf[t] = z, P
    return zp, Pp, zf, Pf, ll


def expect(x, Lam, R, A, Q, mu0, P0, H=0, t0=0, mean=None, sd=None):
    """Every output of dfm_filter_batch for one replicate, in the entry's layouts (packed covariances)."""
    x = np.asarray(x, float)
    T, N = x.shape
    r, k = A.shape
    zp, Pp, zf, Pf, ll = textbook_filter(x, Lam, R, A, Q, mu0, P0)
    mu = np.zeros(N) if mean is None else np.asarray(mean, float)
    s = np.ones(N) if sd is None else np.asarray(sd, float)
    m = zp[:, :r] @ Lam.T
    var = np.einsum("ia,tab,ib->ti", Lam, Pp[:, :r, :r], Lam) + R
    out = dict(z_pred=zp, P_pred=pack(Pp), z_filt=zf, P_filt=pack(Pf), loglik_t=ll, xpred=mu + s * m, verr=s * (x - m),
               vstd=(x - m) / np.sqrt(var))
    if H > 0:
        M, _ = companion(A, Q)
        msfe = np.full((H, N), np.nan); msfe0 = np.full((H, N), np.nan); cnt = np.zeros((H, N), np.int32)
        for h in range(1, H + 1):
            Mh = np.linalg.matrix_power(M, h)
            for i in range(N):
                e2 = x2 = 0.0
                n = 0
                for t in range(t0, T - h):
                    xv = x[t + h, i]
                    if not np.isnan(xv):
                        e2 += (xv - Lam[i] @ (Mh @ zf[t])[:r]) ** 2
                        x2 += xv * xv
                        n += 1
                cnt[h - 1, i] = n
                if n:
                    msfe[h - 1, i] = s[i] ** 2 * e2 / n
                    msfe0[h - 1, i] = s[i] ** 2 * x2 / n
        out.update(msfe=msfe, msfe0=msfe0, cnt=cnt)
    return out


def collapsed_update(zp, Pp, r, b, C, s, n, ld):
    """filter_kernel's update, restated: nothing but W = I + U' C U is factorised.  Returns z_filt, P_filt, loglik_t."""
    S = Pp[:, :r]
    P11 = S[:r]
    U = psd_root(P11)
    W = np.eye(r) + U.T @ C @ U
    Lw = np.linalg.cholesky(W)
    Ginv = np.eye(r) - C @ U @ np.linalg.solve(W, U.T)
    f = zp[:r]
    a = b - C @ f
    ga = Ginv @ a
    GC = Ginv @ C
    GC = 0.5 * (GC + GC.T)
    z = zp + S @ ga
    P = Pp - S @ GC @ S.T
    ll = -0.5 * (n * LOG2PI + ld + 2.0 * np.log(np.diag(Lw)).sum() + s - 2.0 * b @ f + f @ C @ f - a @ P11 @ ga)
    return z, 0.5 * (P + P.T), ll


def params_for(B, N, T, r, p, missing=0.0, first=0):
    """Panels [B, T, N] and parameters of a case: drawn on max(T, 100) rows (the VAR start needs them), the panel cut to T."""
    x, st = synth(B, N, max(T, 100), r, p, missing=missing, first=first)
    return np.ascontiguousarray(x[:, :T]), st


# ---------------------------------------------------------------------------------------------------- the fill's launch geometry
def fill_launch(B, N, r, T, aligned=True):
    """launch_filter_fill (filter.hip): SP = 2 for even N in a register bucket <= 16 with 16-byte aligned pointers;
    filter_fill_kernel<RB, SP> over T rows of r + r (r + 1) / 2 staged doubles (f_pred and the packed P11)."""
    rb = pg.rb_bucket(r)
    sp = 2 if N % 2 == 0 and rb <= 16 and aligned else 1
    call = ((N + sp - 1) // sp, r + r * (r + 1) // 2, T, FT_MAX_THREADS, FT_LDS)
    return pg._summary("filter_fill_kernel", call, lambda g: (B * g["nchunk"] * g["nsblk"], 1, 1), SP=sp, RB=rb, vec=sp == 2)


def fill_classes(B, N, r, T, aligned=True):
    g = fill_launch(B, N, r, T, aligned)
    out = {"nsblk=1" if g["nsblk"] == 1 else "nsblk=2" if g["nsblk"] == 2 else "nsblk>=3", "vec" if g["vec"] else "scalar",
           f"rb={g['RB']}"}
    if g["idle_last"]:
        out.add("idle_last_block")
    if g["RC"] == 8 * g["G"]:
        out.add("rc=8G")
    if g["cap_binds"]:
        out.add("rc=cap")
    if g["RC"] == T:
        out.add("rc=rows")
    if g["partial_last"]:
        out.add("partial_chunk")
    return out


REQUIRED = {"nsblk=1", "nsblk=2", "nsblk>=3", "idle_last_block", "vec", "scalar", "rc=8G", "rc=cap", "rc=rows", "partial_chunk",
            "rb=4", "rb=8", "rb=16", "rb=32"}

# The GPU case table: (name, r, p, N, T, missing, H, t0, scaled, aligned).  B = 2 everywhere.
SHAPES = [(1, 1), (3, 1), (8, 1), (2, 3), (4, 4), (5, 6), (8, 4), (17, 1), (32, 1)]


def _n_of(r):
    return 24 if r <= 8 else 130 if r == 32 else 40


RECURSION = [(f"r{r}p{p}_T{T}_{'miss' if ms else 'bal'}", r, p, _n_of(r), T, ms, 3, 0, True, True)
             for (r, p) in SHAPES for T in (1, 2, 37) for ms in (0.0, 0.1)]
RECURSION.append(("r4p4_T230_miss", 4, 4, 24, 230, 0.1, 3, 100, True, True))
CROSS = [(f"N{N}_r8", 8, 1, N, 20, 0.1 if N % 2 else 0.0, 2, 3, N != 7, True) for N in (1, 7, 130, 200, 257)]
CROSS += [("N1024_r8", 8, 1, 1024, 9, 0.0, 1, 0, True, True), ("N256_r32", 32, 1, 256, 9, 0.1, 1, 0, False, True),
          ("N1024_r8_misaligned", 8, 1, 1024, 9, 0.1, 1, 0, True, False), ("N200_r12", 12, 1, 200, 20, 0.1, 2, 3, True, True),
          ("N130_r8_misaligned", 8, 1, 130, 20, 0.0, 2, 3, False, False)]
EVAL = [(f"eval_H{H}_t{t0}", 3, 2, 24, 12, 0.1, H, t0, True, True) for (H, t0) in ((0, 0), (1, 0), (5, 0), (5, 11), (5, 4), (9, 6))]
CASES = RECURSION + CROSS + EVAL
CASE_KEYS = ("name", "r", "p", "N", "T", "missing", "H", "t0", "scaled", "aligned")


def case_dict(row):
    return dict(zip(CASE_KEYS, row))


def missing_classes():
    seen = set()
    for row in CASES:
        c = case_dict(row)
        seen |= fill_classes(2, c["N"], c["r"], c["T"], c["aligned"])
    return REQUIRED - seen
