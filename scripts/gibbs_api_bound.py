#!/usr/bin/env python
"""The figures behind the bound of tests/test_gpu_gibbs.py::test_estimate_bayesian_against_the_em_fit, from the NumPy model alone
(no GPU, about a minute): the panel, the window, the EM fit (oracle PCA start, 20 iterations) and the sampler's settings are those
of the test; the expectation model of tests/gibbs_expect.py runs the 4 chains x (300 + 300) sweeps on the header's stream.
Prints the distance of the posterior-mean common component from the smoothed common component at the EM estimate (the test's
API_MODEL_DISTANCE), the model's split-R-hat, and how far two runs drift apart whose starts differ by 1e-9 (the test's margin)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamic_factor_models_amd import api, bayes  # noqa: E402
from oracle import kalman_oracle as ko  # noqa: E402
from tests import gibbs_expect as ge  # noqa: E402

N, T, r, CHAINS, BURN, KEPT, SEED = 30, 120, 2, 4, 300, 300, 77
KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")

x, _ = ko.synth_replicate(7, N, T, r)
m = api.DFMModel(x, np.ones(N, int), 20, 40, 1, T, 0, r, 1e-8, 1, 1)
cols, z, mu, sd = api._forecast_inputs(m, T)
start, _ = ko.pca_init(z, r)
ep, _, _ = ko.em(z, start, max_iter=20, tol=0.0)
prior = bayes.check_prior(None, r, 1, CHAINS)


def run(first, chains):
    out = []
    for b in chains:
        cur = {k: np.array(first[k]) for k in KEYS}
        Ls, Rs, fs = [], [], []
        for j in range(BURN + KEPT):
            w = ge.sweep(z, *[cur[k] for k in KEYS], 1, prior, SEED, j, b)
            cur.update(Lam=w["Lam"], R=w["R"], A=w["A"], Q=w["Q"])
            Ls.append(w["Lam"]); Rs.append(w["R"]); fs.append(w["f"])
        out.append((np.array(Ls), np.array(Rs), np.array(fs)))
    return out


res = run(ep, range(CHAINS))
Ld, Rd, fd = (np.stack([res[b][i][BURN:] for b in range(CHAINS)]) for i in range(3))
post = np.mean([bayes.common_component(Ld[c], fd[c], mu, sd).mean(0) for c in range(CHAINS)], axis=0)
f_em = ko.kfs_pass(z, *[ep[k] for k in KEYS], lag_one=False)["f_smooth"][:, :r]
em_common = mu + sd * (f_em @ ep["Lam"].T)
print(f"API_MODEL_DISTANCE {np.abs(post - em_common).max() / max(1.0, np.abs(em_common).max()):.8f}")
last = bayes.common_component(Ld, fd, mu, sd, rows=[T - 1])[:, :, 0, :]
print(f"split-R-hat: R {bayes.split_rhat(Rd * sd ** 2).max():.4f}, common component (last period) {bayes.split_rhat(last).max():.4f}")
near = {k: np.array(v) for k, v in ep.items()}
near["Lam"] = near["Lam"] + 1e-9 * np.random.default_rng(0).standard_normal(near["Lam"].shape)
near["R"] = near["R"] * (1.0 + 1e-9)
alt = run(near, [0])
print(f"starts 1e-9 apart: loadings stay within {np.abs(alt[0][0] - res[0][0]).max():.2e}, factors within "
      f"{np.abs(alt[0][2] - res[0][2]).max():.2e} over {BURN + KEPT} sweeps")
