"""Expectation model of one sweep of dfm_gibbs_ar_batch (include/dfm_hip.h; csrc/gibbs_ar.hip) on the CPU, in two parts, as
gibbs_expect.py:
  sweep_from_randoms  steps 1-4 of the header for given normals and Gamma attempts (simsmooth_ar_expect for step 1, gibbs_expect's
                      solves, Gamma and VAR block for the rest)
  stream_randoms      those numbers from the header's stream table (oracle/synth_oracle.py's Philox4x32-10)
Besides the draws a sweep reports what decides an accept: the rejected attempts per series of streams 6 and 11, and the smallest
distance of any attempt from its decision boundary, so that tests/test_gibbs_ar_cpu.py can assert that the device cannot decide
an accept differently.  Shared by tests/test_gibbs_ar_cpu.py and tests/test_gpu_gibbs_ar.py."""
import numpy as np

from oracle import synth_oracle as so
from tests import gibbs_expect as ge
from tests import simsmooth_ar_expect as sae
from tests.simsmooth_expect import _pairs

RHO_CAP = 32
KEYS = sae.KEYS                                                  # Lam, sig2, rho, Avar, Q, mu0, P0
STATE = KEYS[:5]


def prior(r, **kw):
    return ge.prior(r, **dict(dict(tau_rho=4.0), **kw))


def used_rows(xo, q):
    """xo [n, N] output rows -> bool [n, N]: t is in U_i when cells t, t-1, .. t-q of series i are all observed."""
    obs = ~np.isnan(xo)
    use = obs.copy()
    for l in range(1, q + 1):
        use[l:] &= obs[:-l]
    use[:q] = False
    return use


def stationary(phi):
    """The step-down (Levinson) recursion of the header: (stationary, min over the steps taken of | |kappa| - 1 |)."""
    c = np.array(phi, float)
    margin = np.inf
    for k in range(len(c), 0, -1):
        kap = c[k - 1]
        margin = min(margin, abs(abs(kap) - 1.0))
        if not abs(kap) < 1.0:
            return False, margin
        c = (c[:k - 1] + kap * c[:k - 1][::-1]) / (1.0 - kap * kap)
    return True, margin


def rho_attempts(key, word, N, q):
    """[RHO_CAP, N, q]: attempt k of series i uses idx = (k N + i) ceil(q / 2) + l / 2, component l mod 2."""
    return _pairs(key, word, RHO_CAP * N, q).reshape(RHO_CAP, N, q)


def stream_randoms(seed, sweep, b, T, N, r, p, q):
    """Every random number of sweep `sweep` of chain b: key = replicate_key(seed, sweep), stream word 16 b + s."""
    key = so.replicate_key(seed, sweep)
    w = 16 * b
    return dict(ss=sae.stream_normals(seed, sweep, 0, b, T, 0, N, r, p, q),     # streams 1, 2, 3, 5
                gam_R=ge.gamma_attempts(key, w + 6, N), E=_pairs(key, w + 7, r * p, r), bart_n=ge.bartlett_normals(key, w + 8, r),
                gam_Q=ge.gamma_attempts(key, w + 9, r), lam_n=_pairs(key, w + 10, N, r), rho_n=rho_attempts(key, w + 11, N, q))


# ---------------------------------------------------------------------- step 2: rho_i | lam_i, sig2_i, F
def rho_posterior(xi, f, lam, sig2, use, q, tau_rho):
    """xi [n] (NaN = missing), use [n]: (L, y) with L L' = S = tau_rho I + sum w w' / sig2 and y = L^-1 sum w e_t / sig2, the sums
    over t in ascending order."""
    e = np.where(np.isnan(xi), 0.0, xi - f @ lam)
    Sww, swe = np.zeros((q, q)), np.zeros(q)
    for t in np.nonzero(use)[0]:
        w = e[t - q:t][::-1]
        Sww += np.outer(w, w)
        swe += w * e[t]
    L = np.linalg.cholesky(tau_rho * np.eye(q) + Sww / sig2)
    return L, ge._lsolve(L, swe / sig2)


def rho_from(L, y, n):
    """A candidate: L^-T (y + n)."""
    return ge._ltsolve(L, y + n)


def draw_rho(L, y, normals, old):
    """normals [RHO_CAP, q].  Returns (rho, rejected attempts, min margin): `old` and RHO_CAP when every attempt is rejected."""
    margin = np.inf
    for k in range(RHO_CAP):
        cand = rho_from(L, y, normals[k])
        ok, mg = stationary(cand)
        margin = min(margin, mg)
        if ok:
            return cand, k, margin
    return np.array(old, float), RHO_CAP, margin


# ---------------------------------------------------------------------- step 3: sig2_i, lam_i | rho_i, F
def quasi_difference(xi, f, rho, use):
    """(x~ [n_i], f~ [n_i, r]) over U_i."""
    q = len(rho)
    x0 = np.where(np.isnan(xi), 0.0, xi)
    tt = np.nonzero(use)[0]
    xt = np.array([x0[t] - sum(rho[l] * x0[t - 1 - l] for l in range(q)) for t in tt])
    ft = np.array([f[t] - sum(rho[l] * f[t - 1 - l] for l in range(q)) for t in tt]).reshape(len(tt), f.shape[1])
    return xt, ft


def gamma_margin(a, z, u, first):
    """The smallest distance from the accept boundary over the attempts 0 .. first of every item: |log u - rhs| where v > 0,
    |v| where the attempt fails on v <= 0."""
    z, u = np.asarray(z, float), np.asarray(u, float)
    n = z.shape[1]
    a = np.broadcast_to(np.asarray(a, float), (n,))
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    t = 1.0 + c * z
    v = t * t * t
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(v > 0.0, np.abs(np.log(u) - (0.5 * z * z + d - d * v + d * np.log(np.where(v > 0.0, v, 1.0)))), np.inf)
    m = np.minimum(m, np.abs(t))
    took = np.arange(z.shape[0])[:, None] <= np.minimum(first, z.shape[0] - 1)[None, :]
    return float(np.where(took, m, np.inf).min()) if n else np.inf


def draw_series(xo, f, Lam, sig2, rho, pr, rnd):
    """Steps 2 and 3 for every series of one chain: xo [n, N] output rows."""
    n, N = xo.shape
    r, q = Lam.shape[1], rho.shape[1]
    use = used_rows(xo, q)
    rho1, att_rho, m_rho = np.empty((N, q)), np.empty(N, int), np.inf
    Ls, ys, a, bb = [], [], np.empty(N), np.empty(N)
    for i in range(N):
        L, y = rho_posterior(xo[:, i], f, Lam[i], sig2[i], use[:, i], q, pr["tau_rho"])
        rho1[i], att_rho[i], mg = draw_rho(L, y, rnd["rho_n"][:, i], rho[i])
        m_rho = min(m_rho, mg)
        xt, ft = quasi_difference(xo[:, i], f, rho1[i], use[:, i])
        L, y, xx = ge.load_posterior(ft, xt, pr["tau_lam"])
        Ls.append(L); ys.append(y)
        a[i] = 0.5 * (pr["nu_R"] + use[:, i].sum())
        bb[i] = 0.5 * (pr["nu_R"] * pr["s_R"] + xx - y @ y)
    g, att_R = ge.gamma_mt(a, *rnd["gam_R"])
    s2 = bb / g
    Lam1 = np.stack([ge.lam_from(Ls[i], ys[i], s2[i], rnd["lam_n"][i]) for i in range(N)])
    return dict(Lam=Lam1, sig2=s2, rho=rho1, att_R=att_R, att_rho=att_rho, n_i=use.sum(0), margin_rho=m_rho,
                margin_gamma=gamma_margin(a, *rnd["gam_R"], att_R))


# ---------------------------------------------------------------------- one sweep
def sweep_from_randoms(x, Lam, sig2, rho, A, Q, mu0, P0, pr, rnd):
    """One sweep of one chain from the state (Lam, sig2, rho, A, Q); x [T, N].  Returns dict(Lam, sig2, rho, A, Q, f, att_R [N],
    att_rho [N] (RHO_CAP: the cap, rho_i unchanged), att_Q [r], n_i [N], margin_rho, margin_gamma)."""
    q = rho.shape[1]
    p = A.shape[1] // Lam.shape[1]
    f, _ = sae.draw_from_normals(x, Lam, sig2, rho, A, Q, mu0, P0, 0, rnd["ss"])
    out = draw_series(x[q:], f, Lam, sig2, rho, pr, rnd)
    A1, Q1, att_Q = ge.draw_var(f, p, pr, rnd["E"], rnd["bart_n"], rnd["gam_Q"])
    nQ = pr["nu_Q"] + (f.shape[0] - p)
    mq = gamma_margin(0.5 * (nQ - np.arange(Q.shape[0])), *rnd["gam_Q"], att_Q)
    return dict(out, A=A1, Q=Q1, f=f, att_Q=att_Q, margin_gamma=min(out["margin_gamma"], mq))


def sweep(x, Lam, sig2, rho, A, Q, mu0, P0, pr, seed, sweep_index, b):
    """sweep_from_randoms on the header's stream: what sweep `sweep_index` of chain b returns from this state."""
    T, N = x.shape
    r = Lam.shape[1]
    return sweep_from_randoms(x, Lam, sig2, rho, A, Q, mu0, P0, pr,
                              stream_randoms(seed, sweep_index, b, T, N, r, A.shape[1] // r, rho.shape[1]))
