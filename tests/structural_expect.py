"""Expectation model of dfm_irf_batch and dfm_histdecomp_batch (include/dfm_hip.h) on the CPU: the header's definitions written
straight from the formulas with numpy.linalg (companion-matrix powers, solves), sharing nothing with csrc/structural.hip.  The
oracle's smoother supplies f_t|T.  Shared by tests/test_structural_cpu.py and tests/test_gpu_structural.py."""
import numpy as np

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests.simsmooth_expect import psd_root      # lower root with the zero-column rule: a pivot <= 1e-12 trace gives a zero column


def impact(Lam, Q, named=None):
    """S with eta = S u: Ln^-1 chol(Ln Q Ln') for Ln = Lam[named], chol(Q) without named series."""
    if named is None:
        return psd_root(Q)
    Ln = Lam[np.asarray(named)]
    return np.linalg.solve(Ln, psd_root(Ln @ Q @ Ln.T))


def companion(A):
    r, k = A.shape
    M = np.zeros((k, k))
    M[:r] = A
    M[r:, :k - r] = np.eye(k - r)
    return M


def thetas(A, S, H):
    """Theta_h = Psi_h S, h = 0 .. H-1, Psi_h the top-left block of the companion matrix's h-th power.  [H, r, r]"""
    r = S.shape[0]
    M = companion(A)
    return np.stack([np.linalg.matrix_power(M, h)[:r, :r] @ S for h in range(H)])


def greedy_named(Lam):
    """r rows of Lam by greedy pivoting: the row with the largest residual norm after projecting out the rows chosen so far."""
    r = Lam.shape[1]
    res = Lam.astype(float).copy()
    out = []
    for _ in range(r):
        nrm = np.linalg.norm(res, axis=1)
        nrm[out] = -1.0
        i = int(np.argmax(nrm))
        out.append(i)
        q = res[i] / np.linalg.norm(res[i])
        res = res - np.outer(res @ q, q)
    return np.array(out, dtype=np.int32)


def irf_fevd(Lam, A, Q, R, H, sd=None, named=None, cum=None, unit_effect=False):
    """One replicate.  Returns dict(irf [r, H, N], fevd [r+1, H, N], num [r, H, N] the sums before normalisation,
    idio [H, N])."""
    N, r = Lam.shape
    S = impact(Lam, Q, named)
    Th = thetas(A, S, H)
    s = np.ones(N) if sd is None else np.asarray(sd, float)
    c = np.zeros(N, bool) if cum is None else np.asarray(cum) != 0
    resp = np.einsum("im,hmk->khi", Lam, Th)                      # lam_i' Theta_h e_k
    resp = np.where(c, np.cumsum(resp, axis=1), resp)
    irf = s * resp
    if unit_effect:
        nm = np.asarray(named)
        irf = irf / irf[np.arange(r), 0, nm][:, None, None]
    num = np.cumsum(resp ** 2, axis=1)
    idio = np.where(c, np.arange(1, H + 1)[:, None] * R, np.broadcast_to(R, (H, N)))
    tot = num.sum(axis=0) + idio
    return dict(irf=irf, fevd=np.concatenate([num, idio[None]]) / tot, num=num, idio=idio)


def smooth(x, Lam, R, A, Q, mu0, P0, p=1):
    """f_t|T [T, r] and the log-likelihood from the oracle's smoother."""
    r = Lam.shape[1]
    out = ko.kfs_pass(x, Lam, R, A, Q, mu0, P0, lag_one=False) if p == 1 else vo.kfs_pass_varp(x, Lam, R, A, Q, mu0, P0, p)
    return out["f_smooth"][:, :r], out["loglik"]


def histdecomp(f, Lam, A, Q, sd=None, named=None):
    """One replicate from smoothed factors f [T, r].  Returns dict(hd [r+1, T, N], shocks [T, r], paths [r+1, T, r])."""
    T, r = f.shape
    p = A.shape[1] // r
    S = impact(Lam, Q, named)
    s = np.ones(Lam.shape[0]) if sd is None else np.asarray(sd, float)
    Aj = [A[:, j * r:(j + 1) * r] for j in range(p)]
    u = np.zeros((T, r))
    for t in range(p, T):
        eta = f[t] - sum(Aj[j] @ f[t - 1 - j] for j in range(p))
        u[t] = np.linalg.solve(S, eta)
    c = np.zeros((r + 1, T, r))
    c[r, :p] = f[:p]
    for t in range(p, T):
        for k in range(r + 1):
            c[k, t] = sum(Aj[j] @ c[k, t - 1 - j] for j in range(p))
            if k < r:
                c[k, t] += S[:, k] * u[t, k]
    return dict(hd=s * np.einsum("ktm,im->kti", c, Lam), shocks=u, paths=c)


def rotate(Lam, A, Q, M):
    """Lam M^-1, M A_j M^-1, M Q M'."""
    r = Lam.shape[1]
    Mi = np.linalg.inv(M)
    p = A.shape[1] // r
    return Lam @ Mi, np.hstack([M @ A[:, j * r:(j + 1) * r] @ Mi for j in range(p)]), M @ Q @ M.T


KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")


def synth(B, N, T, r, p=1, missing=0.0, first=0):
    """The oracle's synthetic panels [B, T, N] and parameters (A = [A_1 .. A_p]), as the forecast tests draw them."""
    if p == 1:
        reps = [ko.synth_replicate(first + b, N, T, r, missing=missing) for b in range(B)]
        return np.stack([x for x, _ in reps]), {k: np.stack([q[k] for _, q in reps]) for k in KEYS}
    xs, qs = [], []
    for b in range(B):
        x = vo.synth_varp(first + b, N, T, r, p, missing=missing)
        q, _ = vo.varp_init(np.nan_to_num(x), r, p)
        xs.append(x); qs.append(dict(q, A=q["Avar"]))
    return np.stack(xs), {k: np.stack([q[k] for q in qs]) for k in KEYS}
