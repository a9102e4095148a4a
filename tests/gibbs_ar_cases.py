"""The case table of tests/test_gpu_gibbs_ar.py, shared with tests/test_gibbs_ar_cpu.py (which asserts from the model that the table
meets a rejected rho attempt, a rejected Gamma attempt, a series without a usable row and the rho cap, and that no accept is
decided within 1e-6 of its boundary).  Every case runs SWEEPS sweeps of B chains.  Together: q = 1 .. 4; p below, at and above
q + 1; r = 1, 4 and 8 with k = 32; N = 1, 64, 65, 139 and 257 (two series blocks); n = p + 1; a balanced panel; every pattern class
of forecast_ar_expect.apply_pattern; a series never observed and one with 0 < n_i < r; A0 with DFM_F_SINGULAR_Q; the rho cap."""
import functools

import numpy as np

from tests import forecast_ar_expect as fe
from tests import gibbs_ar_expect as gae

B, SWEEPS = 2, 3
KEYS = gae.KEYS

# name: (N, T, r, p, q, first pattern kind (None: balanced), seed, what it reaches)
CASES = {
    "q1_n1_gap": (1, 40, 1, 1, 1, 4, 201, "N = 1; p below q + 1"),
    "q2_p_eq_n64": (64, 40, 2, 3, 2, 0, 202, "p = q + 1; a full wave"),
    "q3_r8_n65": (65, 41, 8, 1, 3, 3, 203, "bucket 8 with k = 32; idle lanes of a second wave; two row chunks"),
    "q4_p_gt_n139": (139, 40, 1, 6, 4, 1, 204, "p above q + 1; q = 4"),
    "q1_r4_n257_two_blocks": (257, 40, 4, 2, 1, 2, 205, "a second series block"),
    "q2_n_min": (6, 4, 1, 1, 2, 4, 206, "n = p + 1: no usable row at all"),
    "q3_balanced": (10, 24, 2, 2, 3, None, 207, "a balanced panel"),
    "q1_r4_few_rows": (12, 30, 4, 1, 1, None, 208, "a series never observed and one with 0 < n_i < r"),
    "q2_a0_singular_q": (20, 40, 2, 1, 2, 0, 209, "A0 path; covariance-form pass"),
    "q4_tau1_cap": (139, 40, 1, 6, 4, 1, 210, "tau_rho = 1: 32 rejected rho attempts"),
}


@functools.lru_cache(maxsize=None)
def build(name):
    """dict(panel [B,T,N], st (KEYS -> [B,..]), dims (N, T, r, p, q), prior, may_have_missing, singular_q, seed, kinds).  Cached:
    treat it as read only."""
    N, T, r, p, q, first, seed, _ = CASES[name]
    xs, sts, kinds = [], [], set()
    for b in range(B):
        x, st, _ = fe.synth(b + 3, max(N, r + 2), max(T, 3 * r + 12), r, p, q)
        x = np.ascontiguousarray(x[:T, :N])
        st = dict(st, Lam=st["Lam"][:N], sig2=st["sig2"][:N], rho=st["rho"][:N])
        if first is not None:
            kinds |= fe.apply_pattern(x, q, first + b)
        xs.append(x); sts.append(st)
    panel = np.stack(xs)
    pr = gae.prior(r)
    singular_q = False
    if name == "q1_r4_few_rows":
        panel[:, :, 3] = np.nan                                 # never observed
        panel[:, :10, 5] = np.nan                               # panel rows 10 .. 12 only: output rows 9 .. 11, n_i = 2 < r
        panel[:, 13:, 5] = np.nan
    if name == "q2_a0_singular_q":
        singular_q = True
        rng = np.random.default_rng(seed)
        pr = gae.prior(r, A0=0.5 * np.eye(r)[None] + 0.1 * rng.standard_normal((B, r, r)), tau_A=3.0, s_Q=0.7, nu_Q=r + 4.5,
                       tau_rho=2.5, nu_R=3.5, s_R=0.8, tau_lam=2.0)
    if name == "q4_tau1_cap":
        pr = gae.prior(r, tau_rho=1.0)
    return dict(panel=panel, st={k: np.stack([s[k] for s in sts]) for k in KEYS}, dims=(N, T, r, p, q), prior=pr,
                may_have_missing=bool(np.isnan(panel).any()), singular_q=singular_q, seed=20261020 + seed, kinds=kinds)


def chain_prior(c, b):
    pr = c["prior"]
    return pr if pr["A0"] is None else dict(pr, A0=pr["A0"][b])


@functools.lru_cache(maxsize=None)
def model_chains(name):
    """The model's own chains of the case: [b][j] -> the dict of gibbs_ar_expect.sweep, sweep j started from the model's state after
    sweep j - 1.  Cached (the CPU tests share it)."""
    c = build(name)
    out = []
    for b in range(B):
        cur = {k: c["st"][k][b] for k in KEYS}
        sweeps = []
        for j in range(SWEEPS):
            o = gae.sweep(c["panel"][b], *[cur[k] for k in KEYS], chain_prior(c, b), c["seed"], j, b)
            sweeps.append(o)
            cur = dict(cur, Lam=o["Lam"], sig2=o["sig2"], rho=o["rho"], Avar=o["A"], Q=o["Q"])
        out.append(sweeps)
    return out
