"""CPU checks of the expectation model of dfm_gibbs_batch (tests/gibbs_expect.py), which tests/test_gpu_gibbs.py holds the kernels
against: the conjugate draws against the textbook posteriors computed with np.linalg, the Gamma and Bartlett generators on the
header's fixed stream against their known moments, the prior limits, and the Gamma rejections the GPU case table has to contain.

Attained (this file prints them with -s): the affine parts meet the textbook posteriors to 2.2e-16 (loadings) and 1.9e-16 (VAR)
of the 1e-10 bound; Gamma z-scores (mean, variance) on 40 000 draws: a = 1 (1.62, 1.34), a = 2.5 (1.91, 1.56), a = 60 (1.43, 2.04);
the largest |z| over the entries of E[Q] (1200 draws, r = 3, nu = 12) is 1.61; the GPU case table meets 13 items with a rejected
attempt in stream 6 and 1 in stream 9."""
import numpy as np
import pytest

from oracle import synth_oracle as so
from tests import gibbs_cases as gc
from tests import gibbs_expect as ge

BOUND = 1e-10                                                 # tests/test_simsmooth_cpu.py's bound for the same kind of identity


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def test_loadings_draw_is_the_textbook_posterior():
    rng = np.random.default_rng(0)
    n, r, tau, Ri = 40, 5, 1.3, 0.7
    fi, xi = rng.standard_normal((n, r)), rng.standard_normal(n)
    L, y, xx = ge.load_posterior(fi, xi, tau)
    S = tau * np.eye(r) + fi.T @ fi
    m = np.linalg.solve(S, fi.T @ xi)
    base = ge.lam_from(L, y, Ri, np.zeros(r))
    G = np.stack([ge.lam_from(L, y, Ri, e) - base for e in np.eye(r)], axis=1)
    mid = ge.lam_from(L, y, Ri, 0.5 * np.ones(r))
    errs = (_rel(base, m), _rel(G @ G.T, Ri * np.linalg.inv(S)), _rel(mid, base + 0.5 * G.sum(1)),
            abs(y @ y - m @ S @ m) / (m @ S @ m))
    print("loadings: intercept, G G', affinity, m'Sm:", errs)
    assert max(errs) < BOUND, errs


def test_var_draw_is_the_textbook_posterior():
    rng = np.random.default_rng(1)
    T, r, p = 50, 3, 2
    k = r * p
    f = rng.standard_normal((T, r))
    A0 = 0.2 * rng.standard_normal((r, k))
    pr = ge.prior(r, A0=A0, tau_A=2.5)
    L, M, C, n = ge.var_posterior(f, p, pr)
    Y = f[p:]
    Z = np.array([np.concatenate([f[t - 1 - l] for l in range(p)]) for t in range(p, T)])
    S = pr["tau_A"] * np.eye(k) + Z.T @ Z
    Mt = np.linalg.solve(S, pr["tau_A"] * A0.T + Z.T @ Y)
    Psi = pr["s_Q"] * np.eye(r) + Y.T @ Y + pr["tau_A"] * A0 @ A0.T - Mt.T @ S @ Mt
    Gq = rng.standard_normal((r, r))                          # any root of Q
    Q = Gq @ Gq.T
    vec = lambda At: At.T.reshape(-1, order="F")              # vec(A') of A [r, k]
    base = vec(ge.a_from(L, M, Gq, np.zeros((k, r))))
    J = np.empty((k * r, k * r))
    for e in range(k * r):
        E = np.zeros(k * r); E[e] = 1.0
        J[:, e] = vec(ge.a_from(L, M, Gq, E.reshape(k, r, order="F"))) - base
    errs = (_rel(base, Mt.reshape(-1, order="F")), _rel(J @ J.T, np.kron(Q, np.linalg.inv(S))), _rel(C @ C.T, Psi), float(n != T - p))
    print("VAR: intercept, J J', Psi:", errs)
    assert max(errs) < BOUND, errs


@pytest.mark.parametrize("a", [1.0, 2.5, 60.0])
def test_gamma_moments_on_the_fixed_stream(a):
    n = 40000
    g, att = ge.gamma_mt(a, *ge.gamma_attempts(so.replicate_key(11, 0), 6, n))
    assert att.max() < ge.GAMMA_CAP
    z_mean = (g.mean() - a) / np.sqrt(a / n)
    z_var = (g.var(ddof=1) - a) / np.sqrt((2.0 * a * a + 6.0 * a) / n)      # mu4 - sigma^4 = 2 a^2 + 6 a
    print(f"Gamma({a}): z_mean {z_mean:.2f} z_var {z_var:.2f}, rejected {att.sum() / n:.4f} per item")
    assert abs(z_mean) < 5.0 and abs(z_var) < 5.0, (z_mean, z_var)


def test_inverse_wishart_mean_on_the_fixed_stream():
    r, nu, M = 3, 12.0, 1200
    rng = np.random.default_rng(2)
    W = rng.standard_normal((r, r))
    Psi = W @ W.T + np.eye(r)
    C = np.linalg.cholesky(Psi)
    Qs = np.empty((M, r, r))
    for j in range(M):
        key = so.replicate_key(5, j)
        BT, att = ge.bartlett(nu, ge.bartlett_normals(key, 8, r), ge.gamma_attempts(key, 9, r))
        G = ge.q_root(C, BT)
        Qs[j] = G @ G.T
    d = nu - r
    dd = np.diag(Psi)
    var = ((d + 1.0) * Psi ** 2 + (d - 1.0) * np.outer(dd, dd)) / (d * (d - 1.0) ** 2 * (d - 3.0))   # Var of IW(Psi, nu) entries
    z = (Qs.mean(0) - Psi / (d - 1.0)) / np.sqrt(var / M)
    print("E[Q] z-scores:", np.round(z, 2).tolist())
    assert np.abs(z).max() < 5.0, z


def test_series_without_observed_cells_draws_from_the_prior():
    rng = np.random.default_rng(3)
    T, N, r = 30, 4, 3
    x = rng.standard_normal((T, N))
    x[:, 2] = np.nan
    f = rng.standard_normal((T, r))
    pr = ge.prior(r, tau_lam=1.7, nu_R=5.0, s_R=0.6)
    rnd = ge.stream_randoms(9, 0, 0, T, N, r, 1)
    Lam, R, att = ge.draw_loadings(x, f, pr, rnd["lam_n"], rnd["gam_R"])
    g, _ = ge.gamma_mt(0.5 * pr["nu_R"], rnd["gam_R"][0][:, 2:3], rnd["gam_R"][1][:, 2:3])
    assert abs(R[2] - 0.5 * pr["nu_R"] * pr["s_R"] / g[0]) < 1e-14
    assert np.abs(Lam[2] - np.sqrt(R[2] / pr["tau_lam"]) * rnd["lam_n"][2]).max() < 1e-14


def test_tight_priors_pin_the_draws_to_the_prior_means():
    rng = np.random.default_rng(4)
    T, N, r, p = 40, 6, 2, 2
    x = rng.standard_normal((T, N))
    f = rng.standard_normal((T, r))
    A0 = 0.3 * rng.standard_normal((r, r * p))
    pr = ge.prior(r, tau_lam=1e12, tau_A=1e12, A0=A0)
    rnd = ge.stream_randoms(10, 0, 0, T, N, r, p)
    Lam, R, _ = ge.draw_loadings(x, f, pr, rnd["lam_n"], rnd["gam_R"])
    A, Q, _ = ge.draw_var(f, p, pr, rnd["E"], rnd["bart_n"], rnd["gam_Q"])
    assert np.abs(Lam).max() < 1e-4 and np.abs(A - A0).max() < 1e-4, (np.abs(Lam).max(), np.abs(A - A0).max())
    assert np.all(R > 0.0) and np.all(np.linalg.eigvalsh(Q) > 0.0)


def test_the_gpu_cases_meet_rejected_gamma_attempts_in_both_streams():
    rej6 = rej9 = 0
    for name in gc.CASES:
        aR, aQ = gc.attempt_counts(name)
        assert aR.max() < ge.GAMMA_CAP and aQ.max() < ge.GAMMA_CAP, name
        rej6 += int((aR > 0).sum())
        rej9 += int((aQ > 0).sum())
    print("items with a rejected attempt: stream 6:", rej6, "stream 9:", rej9)
    assert rej6 >= 1 and rej9 >= 1, (rej6, rej9)


def test_a_sweep_of_the_model_runs_from_the_case_table():
    c = gc.build("odd_r")
    out = ge.sweep(c["panel"][1], *[c["st"][k][1] for k in gc.KEYS], c["p"], c["prior"], c["seed"], 2, 1)
    N, T, r, p = gc.CASES["odd_r"][:4]
    assert out["Lam"].shape == (N, r) and out["A"].shape == (r, r * p) and out["f"].shape == (T, r)
    assert np.all(out["R"] > 0.0) and np.all(np.linalg.eigvalsh(out["Q"]) > 0.0)
    assert np.abs(out["Q"] - out["Q"].T).max() < 1e-14
