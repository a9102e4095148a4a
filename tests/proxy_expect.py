"""Expectation model of dfm_proxyirf_batch (include/dfm_hip.h) on the CPU, NumPy only: the block starts from the oracle's Philox
(oracle.synth_oracle: _block, replicate_key), the moments, the impact vector and the responses written straight from the header's
formulas with numpy.linalg, the smoother from the oracle (tests/structural_expect.smooth, the functions tests/forecast_expect.py
uses).  It shares nothing with csrc/proxy.hip.  Shared by tests/test_proxy_cpu.py and tests/test_gpu_proxy.py."""
import functools

import numpy as np

from oracle import synth_oracle as so
from tests import structural_expect as se

STREAM = 11                      # stream word 16 b + 11
KEYS = se.KEYS


def starts(seed, g, b, n, L):
    """The nb = ceil(n / L) block starts of draw g of replicate b, each in 0 .. n - L."""
    nb = -(-n // L)
    w = so._block(so.replicate_key(seed, g), 16 * b + STREAM, np.arange((nb + 3) // 4)).reshape(-1)[:nb]
    return [(int(x) * (n - L + 1)) >> 32 for x in w]                  # Python integers: no rounding


def positions(seed, g, b, n, L):
    """src(j) as positions into U, j = 0 .. n-1: the blocks laid end to end, the last one cut at n."""
    return np.concatenate([np.arange(s, s + L) for s in starts(seed, g, b, n, L)])[:n]


def used_rows(z, p):
    z = np.asarray(z, float)
    return np.array([t for t in range(p, z.size) if np.isfinite(z[t])], dtype=np.int64)


def etahat(f, A):
    """etahat_t = f_t - sum_j A_j f_{t-j} for t >= p, zero rows before.  [T, r]"""
    T, r = f.shape
    p = A.shape[1] // r
    e = np.zeros((T, r))
    for t in range(p, T):
        e[t] = f[t] - sum(A[:, j * r:(j + 1) * r] @ f[t - 1 - j] for j in range(p))
    return e


def slot(eta, z, Q, lam_norm):
    """(hvec, rel) from the n source rows eta [n, r], z [n]; NaN where kappa > 0 is false."""
    zc = z - z.mean()
    m = eta.T @ zc / z.size
    v = float(zc @ zc) / z.size
    kappa = float(m @ np.linalg.solve(Q, m))
    if not kappa > 0.0:
        return np.full(m.size, np.nan), np.nan
    hvec = m / np.sqrt(kappa)
    if lam_norm @ hvec < 0.0:
        hvec = -hvec
    return hvec, kappa / v


def response_tables(Lam, R, A, Q, H, cum=None):
    """What the slots of one replicate share: Psi_h [H, r, r] and den + idio [H, N] (dfm_irf_batch's sum_k num_k + idio)."""
    e = se.irf_fevd(Lam, A, Q, R, H, cum=cum)
    return se.thetas(A, np.eye(Lam.shape[1]), H), e["num"].sum(axis=0) + e["idio"]


def responses(Lam, tables, hvec, norm, sd=None, cum=None, unit=False):
    """(irf [H, N], fevd [H, N]) of one slot."""
    N = Lam.shape[0]
    Psi, den = tables
    c = np.zeros(N, bool) if cum is None else np.asarray(cum) != 0
    s = np.ones(N) if sd is None else np.asarray(sd, float)
    resp = np.einsum("im,hmk,k->hi", Lam, Psi, hvec)
    resp = np.where(c, np.cumsum(resp, axis=0), resp)
    irf = s * resp
    if unit:
        irf = irf / irf[0, norm] if irf[0, norm] != 0.0 else np.full_like(irf, np.nan)
    return irf, np.cumsum(resp ** 2, axis=0) / den


def run(f, Lam, R, A, Q, H, z, norm, D, L, seed, first, b, sd=None, cum=None, unit=False, want_resp=True):
    """Replicate b of one call, from its smoothed factors f [T, r].  Returns dict(impact [D+1, r], rel [D+1], irf [D+1, H, N],
    fevd [D+1, H, N], shock [T], U, pd: whether Q has a Cholesky root)."""
    T, r = f.shape
    N = Lam.shape[0]
    p = A.shape[1] // r
    z = np.asarray(z, float)
    U = used_rows(z, p)
    n = U.size
    eta = etahat(f, A)
    impact, rel = np.empty((D + 1, r)), np.empty(D + 1)
    tables = response_tables(Lam, R, A, Q, H, cum) if want_resp else None
    irf, fevd = np.full((D + 1, H, N), np.nan), np.full((D + 1, H, N), np.nan)
    for s in range(D + 1):
        src = U if s == 0 else U[positions(seed, first + s - 1, b, n, L)]
        impact[s], rel[s] = slot(eta[src], z[src], Q, Lam[norm])
        if want_resp and np.isfinite(rel[s]):
            irf[s], fevd[s] = responses(Lam, tables, impact[s], norm, sd, cum, unit)
    shock = np.zeros(T)
    shock[p:] = eta[p:] @ np.linalg.solve(Q, impact[0])
    try:
        np.linalg.cholesky(Q)
        pd = True
    except np.linalg.LinAlgError:
        pd = False
    return dict(impact=impact, rel=rel, irf=irf, fevd=fevd, shock=shock, U=U, pd=pd)


def rotate_all(q, M):
    """The parameter set under f -> M f: Lam M^-1, M A_j M^-1, M Q M', M mu0, M P0 M' (blockwise for the companion state)."""
    r = q["Lam"].shape[1]
    p = q["A"].shape[1] // r
    L2, A2, Q2 = se.rotate(q["Lam"], q["A"], q["Q"], M)
    K = np.kron(np.eye(p), M)
    return dict(Lam=L2, R=q["R"], A=A2, Q=Q2, mu0=K @ q["mu0"], P0=K @ q["P0"] @ K.T)


# ------------------------------------------------------------------------------------------------------------ the case table
T_CASE, SEED = 48, 20160415
# (name, r, p, N, cum, sd, unit effect, L)
CASES = [("r1", 1, 2, 7, False, False, False, 1), ("r3p2", 3, 2, 12, True, True, False, 4), ("r4p4", 4, 4, 7, False, False, False, 5),
         ("r8unit", 8, 1, 12, False, False, True, 8), ("r9p2", 9, 2, 10, False, False, False, 3), ("r16p2", 16, 2, 20, False, False, False, 6)]
D_CASE = 9
D_EDGES = (0, 1, 63, 64, 65, 255, 256, 257)          # lane, wave and workgroup edges, counting slot 0
T_LONG = 720                     # r = 8: 715 used rows x 9 doubles > 48 KB, the row table is read from global memory


def case_by_name(name):
    return next(c for c in CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def build(name, missing=0.1, case_seed=0, T=None):
    """One case: B = 2 replicates of ONE panel [T, N] (T = T_CASE unless given) (10 % missing cells) with different parameters (Q with a ridge of a
    tenth of its mean eigenvalue), the second set a perturbation of the first; the instrument from replicate 0's own innovations,
    z_t = a' etahat_t + 0.5 sd(a' etahat) noise_t, NaN in one of the first p rows, in the last row and in a run in the middle (as long as makes n no multiple of L > 1); norm = the
    series with the largest |sd_i lam_i' hvec| of replicate 0's slot 0.  Returns a dict; nothing in it is to be modified."""
    _, r, p, N, cum, sd, unit, L = case_by_name(name)
    T = T_CASE if T is None else T
    x, st = se.synth(1, N, T, r, p, missing=missing, first=3 + case_seed)
    g = np.random.default_rng(100 + case_seed)
    q0 = {k: st[k][0] for k in KEYS}
    # (the synthetic start of a VAR(2) in 16 factors on 48 rows has a rank-deficient Q: a ridge keeps every case positive definite)
    q0["Q"] = q0["Q"] + 0.1 * np.trace(q0["Q"]) / r * np.eye(r)
    q1 = dict(q0)
    q1["Lam"] = q0["Lam"] * (1.0 + 0.05 * g.standard_normal(q0["Lam"].shape))
    q1["A"] = 0.9 * q0["A"]
    G = g.standard_normal((r, r))
    q1["Q"] = q0["Q"] + 0.1 * np.trace(q0["Q"]) / r * (G @ G.T) / r
    q1["R"] = q0["R"] * g.uniform(0.8, 1.25, N)
    params = {k: np.stack([q0[k], q1[k]]) for k in KEYS}
    panel = np.stack([x[0], x[0]])
    fs = [se.smooth(panel[b], *[params[k][b] for k in KEYS], p=p) for b in range(2)]
    eta = etahat(fs[0][0], q0["A"])
    a = g.standard_normal(r)
    s = eta[p:] @ a
    z = np.zeros(T)
    z[p:] = s + 0.5 * s.std() * g.standard_normal(T - p)
    z[:p] = g.standard_normal(p)
    run_len = 3
    while True:
        zz = z.copy()
        zz[p - 1] = np.nan; zz[T - 1] = np.nan; zz[20:20 + run_len] = np.nan
        n = used_rows(zz, p).size
        if L == 1 or n % L != 0:
            break
        run_len += 1
    z = zz
    sdv = g.uniform(0.5, 3.0, (2, N)) if sd else None
    cumv = None
    if cum:
        cumv = (g.random(N) < 0.4).astype(np.int32)
        cumv[0], cumv[1] = 1, 0
    h0, _ = slot(eta[used_rows(z, p)], z[used_rows(z, p)], q0["Q"], q0["Lam"][0])
    norm = int(np.argmax(np.abs((sdv[0] if sd else 1.0) * (q0["Lam"] @ h0))))
    return dict(name=name, r=r, p=p, N=N, T=T, L=L, n=n, unit=unit, panel=panel, params=params, z=z, norm=norm, sd=sdv, cum=cumv,
                f=[f for f, _ in fs], loglik=[ll for _, ll in fs])


def expect(c, H, D, L=None, first=0, seed=SEED, f=None, want_resp=True):
    """The model's outputs for both replicates of case c (from the oracle's smoothed factors, or from f [2, T, r])."""
    out = []
    for b in range(2):
        q = {k: c["params"][k][b] for k in KEYS}
        out.append(run(c["f"][b] if f is None else f[b], q["Lam"], q["R"], q["A"], q["Q"], H, c["z"], c["norm"], D, c["L"] if L is None else L,
                       seed, first, b, sd=None if c["sd"] is None else c["sd"][b], cum=c["cum"], unit=c["unit"], want_resp=want_resp))
    return out
