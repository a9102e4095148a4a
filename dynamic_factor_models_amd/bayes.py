"""Host-side pieces of Bayesian estimation (api.estimate_bayesian): the default prior, its checks, and the summaries of the
chains' draws.  Every draw comes from the Gibbs sampler of libdfmhip.so (csrc/gibbs.hip, include/dfm_hip.h); what is here is
NumPy bookkeeping on its output."""
from __future__ import annotations

import numpy as np

PRIOR_KEYS = ("tau_lam", "nu_R", "s_R", "tau_A", "nu_Q", "s_Q", "A0")


def default_prior(r: int) -> dict:
    """Weakly informative on the standardised panel: lam_i | R_i ~ N(0, R_i I), R_i ~ IG(2, 0.5) (mean 0.5), vec(A') | Q ~
    N(0, Q (x) I), Q ~ IW(0.5 I, r + 2) (mean 0.5 I)."""
    return dict(tau_lam=1.0, nu_R=4.0, s_R=0.25, tau_A=1.0, nu_Q=float(r) + 2.0, s_Q=0.5, A0=None)


def check_prior(prior, r: int, p: int, chains: int) -> dict:
    """`prior` (None: default_prior; a dict overrides single entries) with the header's conditions checked; A0 [r, r p] is
    repeated for every chain, A0 [chains, r, r p] is taken as it is."""
    pr = default_prior(r)
    if prior is not None:
        unknown = set(prior) - set(PRIOR_KEYS)
        if unknown:
            raise ValueError(f"unknown prior entries: {sorted(unknown)}")
        pr.update(prior)
    if not (pr["tau_lam"] > 0 and pr["s_R"] > 0 and pr["tau_A"] > 0 and pr["s_Q"] > 0):
        raise ValueError("prior: tau_lam, s_R, tau_A and s_Q must be > 0")
    if not (pr["nu_R"] >= 2 and pr["nu_Q"] >= r + 1):
        raise ValueError("prior: nu_R >= 2 and nu_Q >= r + 1 are required")
    if pr["A0"] is not None:
        A0 = np.asarray(pr["A0"], dtype=np.float64)
        if A0.shape == (r, r * p):
            A0 = np.broadcast_to(A0, (chains, r, r * p))
        if A0.shape != (chains, r, r * p):
            raise ValueError(f"prior A0 must be [r, r p] or [chains, r, r p], got {A0.shape}")
        pr["A0"] = np.ascontiguousarray(A0)
    return pr


def default_prior_ar(r: int) -> dict:
    """default_prior plus rho_i ~ N(0, I / tau_rho) truncated to the stationary region, tau_rho = 4 (sd 0.5 per coefficient): a
    prior-only series is then stationary with probability 0.96 / 0.82 / 0.65 / 0.49 for q = 1 .. 4, so the sampler's 32 attempts
    fail with probability <= 6e-10; tau_rho = 1 at q = 4 gives 0.09 and does reach the cap."""
    return dict(default_prior(r), tau_rho=4.0)


def check_prior_ar(prior, r: int, p: int, chains: int) -> dict:
    """check_prior for the model with AR idiosyncratic terms (api.estimate_bayesian_ar_idio): default_prior_ar, and tau_rho > 0."""
    pr = dict(prior or {})
    unknown = set(pr) - set(PRIOR_KEYS) - {"tau_rho"}
    if unknown:
        raise ValueError(f"unknown prior entries: {sorted(unknown)}")
    tau_rho = pr.pop("tau_rho", default_prior_ar(r)["tau_rho"])
    if not tau_rho > 0:
        raise ValueError("prior: tau_rho must be > 0")
    return dict(check_prior(pr, r, p, chains), tau_rho=float(tau_rho))


def split_rhat(x: np.ndarray) -> np.ndarray:
    """Split-R-hat of Gelman et al. (2013) for draws x [chains, K, ...]: every chain is cut into two halves, and the pooled
    variance estimate of the 2 chains sequences is compared with their mean within-sequence variance.  NaN with fewer than 4
    draws per chain."""
    x = np.asarray(x, dtype=np.float64)
    C, K = x.shape[:2]
    n = K // 2
    if n < 2:
        return np.full(x.shape[2:], np.nan)
    seq = np.concatenate([x[:, :n], x[:, K - n:]], axis=0)                 # [2 C, n, ...]
    W = seq.var(axis=1, ddof=1).mean(axis=0)
    Bn = seq.mean(axis=1).var(axis=0, ddof=1)                              # B / n
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(((n - 1.0) / n * W + Bn) / W)


def common_component(Lam_draw, f_draw, mu, sd, rows=None):
    """mean_i + sd_i lam_i' f_t for every draw: Lam_draw [..., N, r], f_draw [..., T, r] -> [..., T (or len(rows)), N]."""
    f = f_draw if rows is None else f_draw[..., rows, :]
    return mu + sd * np.einsum("...tr,...nr->...tn", f, Lam_draw)
