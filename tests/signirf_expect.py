"""Expectation model of dfm_signirf_batch (include/dfm_hip.h) on the CPU, NumPy only: the candidate stream from the oracle's
Philox (oracle.synth_oracle: normal2's arithmetic, replicate_key), the Haar factor from numpy.linalg.qr with the sign fix, the base
impact matrix and the Theta tables from tests/structural_expect.py.  It shares nothing with csrc/signirf.hip.  Shared by
tests/test_signirf_cpu.py and tests/test_gpu_signirf.py."""
import numpy as np

from oracle import synth_oracle as so
from tests import structural_expect as se

STREAM = 10                      # stream word 16 b + 10
PIV_TOL = 1e-12


def draw_one(seed, cand, b, r):
    """Z [r, r] of candidate `cand` (= first_cand + m) of replicate b, through oracle.synth_oracle.normal2 itself."""
    n2 = (r * r + 1) // 2
    z0, z1 = so.normal2(so.replicate_key(seed, cand), 16 * b + STREAM, np.arange(n2))
    z = np.empty(2 * n2)
    z[0::2], z[1::2] = z0, z1
    return z[:r * r].reshape(r, r)


def draw(seed, first, M, b, r):
    """Z [M, r, r] of candidates first .. first + M - 1: normal2's arithmetic on all keys at once (draw_one is the check)."""
    n2 = (r * r + 1) // 2
    keys = np.array([so.replicate_key(seed, first + m) for m in range(M)], dtype=np.uint64)
    idx = np.broadcast_to(np.arange(n2, dtype=np.uint64), (M, n2))
    stream = 16 * b + STREAM
    ctr = np.stack([(idx & so.MASK).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                    np.full(idx.shape, stream & 0xFFFFFFFF, dtype=np.uint32),
                    np.full(idx.shape, (stream >> 32) & 0xFFFFFFFF, dtype=np.uint32)], axis=-1)
    key = np.stack([(keys & so.MASK).astype(np.uint32), (keys >> np.uint64(32)).astype(np.uint32)], axis=-1)[:, None, :]
    o = so.philox4x32_10(ctr, key)
    u, v = so._u01(o[..., 0], o[..., 1]), so._u01(o[..., 2], o[..., 3])
    rad = np.sqrt(-2.0 * np.log(u))
    z = np.empty((M, 2 * n2))
    z[:, 0::2], z[:, 1::2] = rad * np.cos(2.0 * np.pi * v), rad * np.sin(2.0 * np.pi * v)
    return z[:, :r * r].reshape(M, r, r)


def haar(Z):
    """(Rot, diag U) of Z = Rot U, U upper triangular with a positive diagonal."""
    Qm, U = np.linalg.qr(Z)
    d = np.where(np.diag(U) < 0.0, -1.0, 1.0)
    return Qm * d, np.abs(np.diag(U))


def base_responses(Lam, A, Q, H, sd=None, named=None, cum=None):
    """(S, resp [H, N, r] = lam_i' Theta_h cumulated where cum, the same times sd)."""
    N = Lam.shape[0]
    S = se.impact(Lam, Q, named)
    Th = se.thetas(A, S, H)
    c = np.zeros(N, bool) if cum is None else np.asarray(cum) != 0
    resp = np.einsum("im,hmk->hik", Lam, Th)
    resp = np.where(c[None, :, None], np.cumsum(resp, axis=0), resp)
    s = np.ones(N) if sd is None else np.asarray(sd, float)
    return S, resp, s[None, :, None] * resp


def judge(out_resp, Rot, restr, r):
    """The flip rule for one candidate.  out_resp [H, N, r]: the base responses as they are output.  Returns (accepted, D [r],
    the smallest restricted |response|)."""
    D = np.ones(r)
    ok, margin = True, np.inf
    restr = np.asarray(restr, dtype=np.int64).reshape(-1, 5)
    for k in range(r):
        rows = restr[restr[:, 1] == k]
        if rows.shape[0] == 0:
            continue
        vals = np.concatenate([sg * (out_resp[h0:h1 + 1, i, :] @ Rot[:, k]) for i, _, h0, h1, sg in rows])
        margin = min(margin, float(np.abs(vals).min()))
        if np.all(vals > 0.0):
            pass
        elif np.all(vals < 0.0):
            D[k] = -1.0
        else:
            ok = False
    return ok, D, margin


def run(Lam, A, Q, R, H, restr, M, K, seed, first, b, sd=None, named=None, cum=None, force=None):
    """Replicate b of one call.  force: {candidate: 0 | 1} replaces the model's verdict on those candidates before the slots are
    filled (for candidates the comparison leaves out).  Returns dict(mask [M], n_accept, cand [K], S [K, r, r], irf [K, r, H, N], fevd [K, r+1, H, N],
    Rot [M, r, r], D [M, r], cond [M] of Z, margin [M] the smallest restricted |response| of the candidate, S0 the base S)."""
    N, r = Lam.shape
    S, resp, out_resp = base_responses(Lam, A, Q, H, sd, named, cum)
    Z = draw(seed, first, M, b, r)
    mask = np.zeros(M, np.int32)
    Rots, Ds, cond, margin = np.empty((M, r, r)), np.ones((M, r)), np.empty(M), np.empty(M)
    for m in range(M):
        Rots[m], piv = haar(Z[m])
        cond[m] = np.linalg.cond(Z[m])
        ok, Ds[m], margin[m] = judge(out_resp, Rots[m], restr, r)
        mask[m] = int(ok and piv.min() > PIV_TOL * np.abs(Z[m]).max())
    for m, v in (force or {}).items():
        mask[m] = v
    acc = np.nonzero(mask)[0]
    cand = np.full(K, -1, np.int32)
    cand[:min(K, acc.size)] = acc[:K]
    c = np.zeros(N, bool) if cum is None else np.asarray(cum) != 0
    idio = np.where(c, np.arange(1, H + 1)[:, None] * R, np.broadcast_to(R, (H, N)))
    So, irf, fevd = np.full((K, r, r), np.nan), np.full((K, r, H, N), np.nan), np.full((K, r + 1, H, N), np.nan)
    for s in range(min(K, acc.size)):
        RD = Rots[cand[s]] * Ds[cand[s]]
        So[s] = S @ RD
        irf[s] = (out_resp @ RD).transpose(2, 0, 1)
        num = np.cumsum((resp @ RD) ** 2, axis=0).transpose(2, 0, 1)
        fevd[s] = np.concatenate([num, idio[None]]) / (num.sum(axis=0) + idio)
    return dict(mask=mask, n_accept=int(acc.size), cand=cand, S=So, irf=irf, fevd=fevd, Rot=Rots, D=Ds, cond=cond, margin=margin,
                S0=S)


def rotated_set(Lam, A, Sm):
    """(Lam S_m, [S_m^-1 A_j S_m], I): the parameter set whose chol(Q) = I responses are those of impact matrix S_m."""
    r = Sm.shape[0]
    p = A.shape[1] // r
    Si = np.linalg.inv(Sm)
    return Lam @ Sm, np.hstack([Si @ A[:, j * r:(j + 1) * r] @ Sm for j in range(p)]), np.eye(r)


def restrictions(series, r):
    """The case table's restrictions on four series (a, b, c, d): a and b positive on shock 0 over h 0-2 and, where r > 1, c
    positive and d negative on shock 1."""
    a, b, c, d = series
    rows = [(a, 0, 0, 2, 1), (b, 0, 0, 2, 1)]
    return rows + [(c, 1, 0, 2, 1), (d, 1, 0, 2, -1)] if r > 1 else rows


CASE_SEED = 5
# (name, N, r, p, the four restricted series).  The series were picked so that, with and without named series, both replicates of
# structural_expect.synth(2, N, ., r, p) have accepted candidates among the first 96 of CASE_SEED (the CPU test holds that).
CASES = [("r4", 12, 4, 1, (0, 1, 2, 3)), ("r3p2", 9, 3, 2, (3, 5, 1, 2)), ("r8", 20, 8, 1, (0, 1, 2, 3)), ("r2", 7, 2, 1, (0, 1, 2, 4)),
         ("r1", 6, 1, 1, (1, 3, 0, 2)), ("r9", 17, 9, 1, (0, 1, 2, 3)), ("r16p2", 24, 16, 2, (0, 2, 3, 4))]
