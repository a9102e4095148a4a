"""The case table of tests/test_gpu_gibbs.py, shared with tests/test_gibbs_cpu.py (which asserts from the model's attempt counts that
the table meets a rejected Gamma attempt in stream 6 and in stream 9).  Every case runs SWEEPS sweeps of B chains."""
import numpy as np

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests import gibbs_expect as ge

B, SWEEPS = 2, 3
KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")

# name: (N, T, r, p, missing, seed, what it reaches)
CASES = {
    "balanced_fused": (60, 90, 8, 1, 0.0, 101, "shared-Gram route, bucket 8"),
    "missing_ragged": (139, 222, 8, 1, 0.1, 102, "chunked route; n_i = 0; odd N"),
    "companion": (37, 64, 4, 4, 0.1, 103, "r p = 16"),
    "odd_r": (5, 20, 3, 2, 0.0, 104, "ceil(r/2) indexing; idle lanes"),
    "two_blocks": (257, 40, 2, 1, 0.1, 105, "workgroup boundary"),
    "two_blocks_balanced": (300, 24, 3, 1, 0.0, 114, "shared root and f rows read by a second series block"),
    "bucket16": (50, 80, 12, 1, 0.1, 106, "bucket 16, a Gram matrix per series"),
    "bucket16_balanced": (50, 80, 12, 1, 0.0, 107, "bucket 16, shared Gram"),
    "wide": (120, 150, 20, 1, 0.1, 108, "tile route; bucket 32, the series' Gram matrix in scratch (one lane per series at every r)"),
    "widest": (80, 100, 32, 1, 0.0, 109, "full 32-bucket"),
    "shortest_var": (20, 3, 2, 2, 0.0, 112, "n = 1; a rejected Gamma attempt in streams 6 and 9"),
    "a0_singular_q": (50, 80, 4, 1, 0.1, 113, "A0 path; covariance-form pass"),
}


def _varp_truth(b, N, r, p):
    rng = np.random.default_rng([7, b, p])
    w = 0.5 ** np.arange(1, p + 1)
    w = 0.85 * w / w.sum()
    sg = np.where(np.arange(p) % 2 == 0, 1.0, -1.0)
    A = np.hstack([np.diag(np.linspace(0.6, 1.0, r)) * w[l] * sg[l] for l in range(p)])
    return dict(Lam=rng.standard_normal((N, r)), R=rng.uniform(0.5, 1.5, N), A=A, Q=np.diag(np.linspace(0.5, 1.0, r)),
                mu0=np.full(r * p, 0.1), P0=np.eye(r * p))


def build(name):
    """dict(panel [B,T,N], st (KEYS -> [B,..]), p, prior, may_have_missing, singular_q, seed)."""
    N, T, r, p, missing, seed, _ = CASES[name]
    if p == 1:
        reps = [ko.synth_replicate(seed + b, N, T, r, missing=missing) for b in range(B)]
        panel = np.stack([x for x, _ in reps])
        st = {k: np.stack([q[k] for _, q in reps]) for k in KEYS}
        st["mu0"] = st["mu0"] + 0.3
    else:
        panel = np.stack([vo.synth_varp(seed + b, N, T, r, p, missing=missing) for b in range(B)])
        tr = [_varp_truth(b, N, r, p) for b in range(B)]
        st = {k: np.stack([q[k] for q in tr]) for k in KEYS}
    pr = ge.prior(r)
    singular_q = False
    if name == "missing_ragged":
        panel[:, -1, :70] = np.nan                              # a ragged edge
        panel[:, :, 17] = np.nan                                # a series with no observed cell
        pr = ge.prior(r, nu_R=3.5, s_R=0.8, tau_lam=2.0)
    if name == "a0_singular_q":
        singular_q = True
        rng = np.random.default_rng(seed)
        pr = ge.prior(r, A0=0.5 * np.eye(r)[None] + 0.1 * rng.standard_normal((B, r, r)), tau_A=3.0, s_Q=0.7, nu_Q=r + 4.5)
    return dict(panel=panel, st=st, p=p, prior=pr, may_have_missing=missing > 0.0, singular_q=singular_q, seed=20261018 + seed)


def attempt_counts(name):
    """Rejected Gamma attempts of the case on the header's stream: (stream 6 [B, SWEEPS, N], stream 9 [B, SWEEPS, r]).  The shape
    parameters depend on the observed-cell counts only, so no sweep has to be run."""
    from oracle import synth_oracle as so
    c = build(name)
    N, T, r, p = CASES[name][:4]
    pr = c["prior"]
    aR = np.zeros((B, SWEEPS, N), int)
    aQ = np.zeros((B, SWEEPS, r), int)
    for b in range(B):
        n_i = (~np.isnan(c["panel"][b])).sum(0)
        for j in range(SWEEPS):
            key = so.replicate_key(c["seed"], j)
            aR[b, j] = ge.gamma_mt(0.5 * (pr["nu_R"] + n_i), *ge.gamma_attempts(key, 16 * b + 6, N))[1]
            aQ[b, j] = ge.gamma_mt(0.5 * (pr["nu_Q"] + (T - p) - np.arange(r)), *ge.gamma_attempts(key, 16 * b + 9, r))[1]
    return aR, aQ
