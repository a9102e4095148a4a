"""Expectation model of one sweep of dfm_gibbs_batch (include/dfm_hip.h) on the CPU, in two parts, as simsmooth_expect.py:
  sweep_from_randoms  steps 1-3 of the header for given normals and Gamma attempts (simsmooth_expect for step 1)
  stream_randoms      those numbers from the header's stream table (oracle/synth_oracle.py's Philox4x32-10)
Shared by tests/test_gibbs_cpu.py (checked against the textbook posteriors with np.linalg) and tests/test_gpu_gibbs.py."""
import numpy as np

from oracle import synth_oracle as so
from tests import simsmooth_expect as se

GAMMA_CAP = 32
PRIOR = dict(tau_lam=1.0, nu_R=4.0, s_R=0.5, tau_A=1.0, nu_Q=None, s_Q=1.0, A0=None)   # nu_Q None: r + 2


def prior(r, **kw):
    q = dict(PRIOR, **kw)
    if q["nu_Q"] is None:
        q["nu_Q"] = r + 2.0
    return q


def _lsolve(L, b):
    """L^-1 b by forward substitution (L lower triangular; b a vector or a matrix of columns)."""
    x = np.array(b, float)
    for i in range(L.shape[0]):
        x[i] = (x[i] - L[i, :i] @ x[:i]) / L[i, i]
    return x


def _ltsolve(L, b):
    """L^-T b by back substitution."""
    x = np.array(b, float)
    for i in range(L.shape[0] - 1, -1, -1):
        x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


# ---------------------------------------------------------------------- Gamma(a, 1), a >= 1: Marsaglia and Tsang (2000)
def gamma_mt(a, z, u):
    """a [n] (or scalar), z / u [GAMMA_CAP, n]: attempt k of item i.  Returns (draw [n], rejected attempts [n]); an item whose
    GAMMA_CAP attempts are all rejected gets d and GAMMA_CAP."""
    z, u = np.asarray(z, float), np.asarray(u, float)
    n = z.shape[1]
    a = np.broadcast_to(np.asarray(a, float), (n,))
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    t = 1.0 + c * z
    v = t * t * t
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (v > 0.0) & (np.log(u) < 0.5 * z * z + d - d * v + d * np.log(np.where(v > 0.0, v, 1.0)))
    first = np.where(ok.any(0), ok.argmax(0), GAMMA_CAP)
    out = np.where(first < GAMMA_CAP, d * v[np.minimum(first, GAMMA_CAP - 1), np.arange(n)], d)
    return out, first


def gamma_attempts(key, word, n_items):
    """(z, u) [GAMMA_CAP, n_items] of the header: attempt k of item i uses m = k n_items + i, z = first normal at idx 2 m,
    u = uniform1 at idx 2 m + 1."""
    m = (np.arange(GAMMA_CAP, dtype=np.uint64)[:, None] * np.uint64(n_items) + np.arange(n_items, dtype=np.uint64)[None, :])
    z, _ = so.normal2(key, word, (2 * m).ravel())
    u = so.uniform1(key, word, (2 * m + 1).ravel())
    return z.reshape(GAMMA_CAP, n_items), u.reshape(GAMMA_CAP, n_items)


def bartlett_normals(key, word, r):
    """[r, r], strict lower part filled: entry (j, c), c < j, is component e mod 2 of the pair at idx e / 2, e = j (j-1)/2 + c."""
    nlow = r * (r - 1) // 2
    out = np.zeros((r, r))
    if nlow:
        z = se._pairs(key, word, 1, nlow)[0]
        for j in range(1, r):
            out[j, :j] = z[j * (j - 1) // 2: j * (j - 1) // 2 + j]
    return out


def stream_randoms(seed, sweep, b, T, N, r, p):
    """Every random number of sweep `sweep` of chain b: key = replicate_key(seed, sweep), stream word 16 b + s."""
    key = so.replicate_key(seed, sweep)
    w = 16 * b
    return dict(ss=se.stream_normals(seed, sweep, 0, b, T, 0, N, r, p),          # streams 1-4
                lam_n=se._pairs(key, w + 5, N, r), gam_R=gamma_attempts(key, w + 6, N),
                E=se._pairs(key, w + 7, r * p, r), bart_n=bartlett_normals(key, w + 8, r), gam_Q=gamma_attempts(key, w + 9, r))


# ---------------------------------------------------------------------- step 2: lam_i, R_i | f
def load_posterior(fi, xi, tau_lam):
    """fi [n_i, r], xi [n_i]: the observed rows of one series.  Returns (L, y, sum x^2) with L L' = S = tau_lam I + fi'fi and
    y = L^-1 fi'xi, so that m = L^-T y and m' S m = y'y."""
    r = fi.shape[1]
    S = tau_lam * np.eye(r) + fi.T @ fi
    L = np.linalg.cholesky(S)
    return L, _lsolve(L, fi.T @ xi), float(xi @ xi)


def lam_from(L, y, Ri, n):
    """lam_i = m + sqrt(R_i) L^-T n = L^-T (y + sqrt(R_i) n)."""
    return _ltsolve(L, y + np.sqrt(Ri) * n)


def draw_loadings(x, f, pr, lam_n, gam_R):
    T, N = x.shape
    r = f.shape[1]
    obs = ~np.isnan(x)
    Ls, ys, a, bb = [], [], np.empty(N), np.empty(N)
    for i in range(N):
        o = obs[:, i]
        L, y, xx = load_posterior(f[o], x[o, i], pr["tau_lam"])
        Ls.append(L); ys.append(y)
        a[i] = 0.5 * (pr["nu_R"] + o.sum())
        bb[i] = 0.5 * (pr["nu_R"] * pr["s_R"] + xx - y @ y)
    g, att = gamma_mt(a, *gam_R)
    R = bb / g
    Lam = np.stack([lam_from(Ls[i], ys[i], R[i], lam_n[i]) for i in range(N)]) if N else np.zeros((0, r))
    return Lam, R, att


# ---------------------------------------------------------------------- step 3: A, Q | f
def var_posterior(f, p, pr):
    """Returns (L, M, C, n): S = tau_A I + Z'Z = L L', M = S^-1 (tau_A A0' + Z'Y), Psi = s_Q I + Y'Y + tau_A A0 A0' - M'SM = C C'."""
    T, r = f.shape
    k = r * p
    Y = f[p:]
    Z = np.hstack([f[p - 1 - l: T - 1 - l] for l in range(p)])
    A0 = np.zeros((r, k)) if pr["A0"] is None else np.asarray(pr["A0"], float)
    S = pr["tau_A"] * np.eye(k) + Z.T @ Z
    L = np.linalg.cholesky(S)
    U = _lsolve(L, pr["tau_A"] * A0.T + Z.T @ Y)
    Psi = pr["s_Q"] * np.eye(r) + Y.T @ Y + pr["tau_A"] * A0 @ A0.T - U.T @ U
    Psi = 0.5 * (Psi + Psi.T)
    return L, _ltsolve(L, U), np.linalg.cholesky(Psi), T - p


def bartlett(nu, bart_n, gam_Q):
    r = bart_n.shape[0]
    g, att = gamma_mt(0.5 * (nu - np.arange(r)), *gam_Q)
    return np.tril(bart_n, -1) + np.diag(np.sqrt(2.0 * g)), att


def q_root(C, BT):
    """G = C B_T^-T (Q = G G')."""
    return _lsolve(BT, C.T).T


def a_from(L, M, G, E):
    """A' = M + L^-T E G'; returns A [r, r p]."""
    return (M + _ltsolve(L, E @ G.T)).T


def draw_var(f, p, pr, E, bart_n, gam_Q):
    L, M, C, n = var_posterior(f, p, pr)
    BT, att = bartlett(pr["nu_Q"] + n, bart_n, gam_Q)
    G = q_root(C, BT)
    return a_from(L, M, G, E), G @ G.T, att


# ---------------------------------------------------------------------- one sweep
def sweep_from_randoms(x, Lam, R, A, Q, mu0, P0, p, pr, rnd):
    """One sweep of one chain from the state (Lam, R, A, Q): returns dict(Lam, R, A, Q, f, att_R [N], att_Q [r]) -- att_*: the
    rejected Gamma attempts per item of streams 6 and 9."""
    f, _ = se.draw_from_normals(x, Lam, R, A, Q, mu0, P0, 0, p, rnd["ss"])
    Lam1, R1, att_R = draw_loadings(x, f, pr, rnd["lam_n"], rnd["gam_R"])
    A1, Q1, att_Q = draw_var(f, p, pr, rnd["E"], rnd["bart_n"], rnd["gam_Q"])
    return dict(Lam=Lam1, R=R1, A=A1, Q=Q1, f=f, att_R=att_R, att_Q=att_Q)


def sweep(x, Lam, R, A, Q, mu0, P0, p, pr, seed, sweep_index, b):
    """sweep_from_randoms on the header's stream: what sweep `sweep_index` of chain b returns from this state."""
    T, N = x.shape
    return sweep_from_randoms(x, Lam, R, A, Q, mu0, P0, p, pr, stream_randoms(seed, sweep_index, b, T, N, Lam.shape[1], p))
